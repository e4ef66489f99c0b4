/*
 * sealhip.h — C ABI of libsealhip.so: the MI355X (gfx950) implementation of Microsoft SEAL's
 * RNS polynomial-arithmetic hot path (negacyclic NTT/INTT, dyadic products, BEHZ base conversion,
 * and the Evaluator ciphertext operations multiply / relinearize / rescale / rotate / mod_switch).
 *
 * The reference has no plugin boundary for this path (seal::Evaluator is a concrete class,
 * native/src/seal/evaluator.h:79-1387); the FFI it does ship is the flat "sealc" export layer that
 * the .NET wrapper P/Invokes (native/src/seal/c/, SEAL_C_FUNC ... HRESULT).  This header follows
 * that layer: the same entry-point names, argument order, HRESULT values and exception-to-HRESULT
 * mapping (native/src/seal/c/defines.h:36-97), so a binding written against sealc's Evaluator_* /
 * Ciphertext_* / KSwitchKeys_* / SEALContext_* functions binds to these with two deliberate
 * differences, both forced by the data living in HBM:
 *   (1) a Ciphertext handle is a DEVICE-RESIDENT BATCH of `batch` ciphertexts that share metadata
 *       (parms_id, size, is_ntt_form, scale): word index of coefficient j of RNS component r of
 *       polynomial p of batch item b is ((p*batch + b)*coeff_modulus_size + r)*N + j — for batch == 1
 *       this is exactly Ciphertext::data() (native/src/seal/ciphertext.h:337-349);
 *   (2) the `void *pool` argument of the sealc signatures is kept for signature compatibility and
 *       must be NULL (a MemoryPoolHandle has no device meaning); work is enqueued on the
 *       Evaluator's HIP stream (Evaluator_SetStream) and is asynchronous until Evaluator_Synchronize
 *       or a Ciphertext_CopyToHost.
 * No C++ type, exception or torch type crosses this boundary.
 *
 * Section 2 ("shl_*") is the finer per-kernel seam, the analogue of the reference's only accelerator
 * hook (the HEXL #ifdef in native/src/seal/util/ntt.cpp:394-475 and polyarithsmallmod.cpp:18-284),
 * taking raw device pointers; it exists for kernel-level parity tests and roofline measurements.
 */
#ifndef SEALHIP_H
#define SEALHIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* HRESULT values of native/src/seal/c/defines.h:36-60 (non-Windows branch). */
typedef long SHL_HRESULT;
#define SHL_S_OK ((SHL_HRESULT)0L)
#define SHL_S_FALSE ((SHL_HRESULT)1L)
#define SHL_E_POINTER ((SHL_HRESULT)0x80004003L)
#define SHL_E_INVALIDARG ((SHL_HRESULT)0x80070057L)
#define SHL_E_OUTOFMEMORY ((SHL_HRESULT)0x8007000EL)
#define SHL_E_UNEXPECTED ((SHL_HRESULT)0x8000FFFFL)
#define SHL_COR_E_IO ((SHL_HRESULT)0x80131620L)             /* std::runtime_error (HIP failure) */
#define SHL_COR_E_INVALIDOPERATION ((SHL_HRESULT)0x80131509L) /* std::logic_error */
#define SHL_E_INVALID_INDEX ((SHL_HRESULT)0x80070585L)      /* HRESULT_FROM_WIN32(ERROR_INVALID_INDEX): std::out_of_range */

#define SHL_FUNC SHL_HRESULT

/* scheme_type (native/src/seal/encryptionparams.h): 0 none, 1 bfv, 2 ckks, 3 bgv */

/* ------------------------------------------------------------------------------------------------
 * 1. sealc-shaped handle API
 * ---------------------------------------------------------------------------------------------- */

/* library / device */
SHL_FUNC SealHip_Version(uint32_t *major, uint32_t *minor, uint32_t *patch);
/* Fails with SHL_COR_E_IO when no gfx950 device is usable: there is no CPU fallback. */
SHL_FUNC SealHip_DeviceInfo(char *name, uint64_t name_capacity, int *compute_units, uint64_t *hbm_bytes);
/* last error text of the calling thread (what() of the C++ exception that produced the HRESULT) */
SHL_FUNC SealHip_LastError(char *outstr, uint64_t *length);

/* CoeffModulus::Create / PlainModulus::Batching (native/src/seal/c/modulus.h CoeffModulus_Create1) */
SHL_FUNC CoeffModulus_Create1(uint64_t poly_modulus_degree, uint64_t length, int *bit_sizes, uint64_t *coeffs);
SHL_FUNC PlainModulus_Batching(uint64_t poly_modulus_degree, int bit_size, uint64_t *value);

/* EncryptionParameters (native/src/seal/c/encryptionparameters.h) */
SHL_FUNC EncParams_Create1(uint8_t scheme, void **enc_params);
SHL_FUNC EncParams_Destroy(void *thisptr);
SHL_FUNC EncParams_SetPolyModulusDegree(void *thisptr, uint64_t degree);
SHL_FUNC EncParams_GetPolyModulusDegree(void *thisptr, uint64_t *degree);
/* sealc passes Modulus handles; here the prime values directly */
SHL_FUNC EncParams_SetCoeffModulus(void *thisptr, uint64_t length, const uint64_t *coeffs);
SHL_FUNC EncParams_GetCoeffModulus(void *thisptr, uint64_t *length, uint64_t *coeffs);
SHL_FUNC EncParams_SetPlainModulus2(void *thisptr, uint64_t plain_modulus);
SHL_FUNC EncParams_GetScheme(void *thisptr, uint8_t *scheme);

/* SEALContext (native/src/seal/c/sealcontext.h, contextdata.h).  Builds the whole modulus-switching
 * chain and uploads NTT tables / RNSTool constants to the current HIP device.  sec_level is accepted
 * for signature compatibility; the HE-standard bound check is the caller's business (BASELINE configs
 * use sec_level_type::none). */
SHL_FUNC SEALContext_Create(void *encryptionParams, bool expand_mod_chain, int sec_level, void **context);
SHL_FUNC SEALContext_Destroy(void *thisptr);
SHL_FUNC SEALContext_KeyParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC SEALContext_FirstParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC SEALContext_LastParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC SEALContext_UsingKeyswitching(void *thisptr, bool *using_keyswitching);
/* ContextData_ChainIndex / ContextData_NextContextData / ContextData_Parms collapsed onto the context */
SHL_FUNC SEALContext_ChainIndex(void *thisptr, uint64_t *parms_id, uint64_t *chain_index);
SHL_FUNC SEALContext_ParmsIdAt(void *thisptr, uint64_t chain_index, uint64_t *parms_id);
SHL_FUNC SEALContext_CoeffModulusAt(void *thisptr, uint64_t chain_index, uint64_t *length, uint64_t *coeffs);
SHL_FUNC SEALContext_TotalCoeffModulusBitCount(void *thisptr, uint64_t chain_index, int *bit_count);
/* parms_ids are computed as the reference does (BLAKE2b-256 of scheme, N, primes, t: encryptionparams.cpp:117-147), so both
 * sides name levels identically; SetParmsId overrides one (kept for bindings that registered them by hand). */
SHL_FUNC SEALContext_SetParmsId(void *thisptr, uint64_t chain_index, uint64_t *parms_id);
/* introspection used by the parity tests: minimal primitive 2N-th root of a pool prime, BEHZ base */
SHL_FUNC SEALContext_NTTRoot(void *thisptr, uint64_t prime_index, uint64_t *root);
SHL_FUNC SEALContext_BaseBsk(void *thisptr, uint64_t chain_index, uint64_t *length, uint64_t *primes);

/* Ciphertext (native/src/seal/c/ciphertext.h) — device-resident batch */
SHL_FUNC Ciphertext_Create3(void *context, void *pool, void **cipher);         /* batch = 1, empty */
SHL_FUNC Ciphertext_CreateBatch(void *context, uint64_t batch, void **cipher); /* empty batch */
SHL_FUNC Ciphertext_Create2(void *copy, void **cipher);
SHL_FUNC Ciphertext_Set(void *thisptr, void *assign);
SHL_FUNC Ciphertext_Destroy(void *thisptr);
SHL_FUNC Ciphertext_Resize1(void *thisptr, void *context, uint64_t *parms_id, uint64_t size);
SHL_FUNC Ciphertext_Size(void *thisptr, uint64_t *size);
SHL_FUNC Ciphertext_BatchCount(void *thisptr, uint64_t *batch);
SHL_FUNC Ciphertext_PolyModulusDegree(void *thisptr, uint64_t *poly_modulus_degree);
SHL_FUNC Ciphertext_CoeffModulusSize(void *thisptr, uint64_t *coeff_modulus_size);
SHL_FUNC Ciphertext_ParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC Ciphertext_IsNTTForm(void *thisptr, bool *is_ntt_form);
SHL_FUNC Ciphertext_SetIsNTTForm(void *thisptr, bool is_ntt_form);
SHL_FUNC Ciphertext_Scale(void *thisptr, double *scale);
SHL_FUNC Ciphertext_SetScale(void *thisptr, double scale);
SHL_FUNC Ciphertext_CorrectionFactor(void *thisptr, uint64_t *correction_factor);
SHL_FUNC Ciphertext_SetCorrectionFactor(void *thisptr, uint64_t correction_factor);
SHL_FUNC Ciphertext_IsTransparent(void *thisptr, bool *result); /* synchronises */
/* device slab access (replaces Ciphertext_GetDataAt/SetDataAt) */
SHL_FUNC Ciphertext_DevicePtr(void *thisptr, uint64_t **data, uint64_t *word_count);
SHL_FUNC Ciphertext_CopyFromHost(void *thisptr, const uint64_t *src, uint64_t word_count);
SHL_FUNC Ciphertext_CopyToHost(void *thisptr, uint64_t *dst, uint64_t word_count);
/* a word range of the slab (the device-resident drop-in keeps the unaligned head / tail of a host buffer current with it) */
SHL_FUNC Ciphertext_CopyWordsToHost(void *thisptr, uint64_t word_offset, uint64_t word_count, uint64_t *dst);
SHL_FUNC Ciphertext_CopyFromDevice(void *thisptr, const uint64_t *src, uint64_t word_count, void *hip_stream);

/* Wire format (native/src/seal/c/ciphertext.h:80-86; Ciphertext::save / load / unsafe_load, native/src/seal/ciphertext.cpp:153-403):
 * the reference's own byte streams - SEALHeader-framed, compr_mode none (0), zlib (1) or zstd (2: libzstd.so.1 at run time;
 * stock reference builds write zstd by default), seeded ciphertexts expanded on load with the
 * reference's Blake2xb / SHAKE256 PRNG - are parsed straight into the device slab and written back from it.  Same argument order
 * as sealc.  Load = UnsafeLoad + is_valid_for (every coefficient reduced, data level).  A handle that is a batch of one behaves
 * exactly like seal::Ciphertext; LoadItem / SaveItem address slot `item` of a larger batch (the first item loaded into an empty
 * batch defines its metadata, later ones must agree).  BGV streams in coefficient form are transformed on load as the reference does. */
SHL_FUNC Ciphertext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC Ciphertext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
SHL_FUNC Ciphertext_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Ciphertext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Ciphertext_LoadItem(void *thisptr, void *context, uint64_t item, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Ciphertext_SaveItem(void *thisptr, uint64_t item, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);

/* SecretKey / Decryptor (native/src/seal/c/secretkey.h, native/src/seal/c/decryptor.h:16-24; seal::Decryptor::decrypt,
 * native/src/seal/decryptor.cpp:79-233): the phase c_0 + c_1 s + ... on the NTT engine, then RNSTool::decrypt_scale_and_round (BFV),
 * decrypt_modt (BGV) or nothing (CKKS: the NTT-form plaintext a CKKSEncoder::decode expects).  SecretKey_Set takes
 * SecretKey::data().data() (L*N words, key level, NTT form); SecretKey_Load the serialized key.  Decryptor_Decrypt is
 * seal::Decryptor::decrypt for a batch of one; Decryptor_DecryptBatch decrypts every item of a batch into caller-owned device
 * memory, untrimmed: [batch][K][N] words (CKKS) or [batch][N] (BFV / BGV). */
SHL_FUNC SecretKey_Create(void *context, void **secret_key);
SHL_FUNC SecretKey_Destroy(void *thisptr);
SHL_FUNC SecretKey_Set(void *thisptr, const uint64_t *host_words, uint64_t word_count);
SHL_FUNC SecretKey_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC SecretKey_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Decryptor_Create(void *context, void *secret_key, void **decryptor);
SHL_FUNC Decryptor_Destroy(void *thisptr);
SHL_FUNC Decryptor_Decrypt(void *thisptr, void *encrypted, void *destination);
SHL_FUNC Decryptor_InvariantNoiseBudget(void *thisptr, void *encrypted, int *invariant_noise_budget); /* BFV / BGV, batch of one */
SHL_FUNC Decryptor_DecryptBatchWords(void *thisptr, void *encrypted, uint64_t *word_count);
SHL_FUNC Decryptor_DecryptBatch(void *thisptr, void *encrypted, uint64_t *device_out, uint64_t word_count);

/* CKKSEncoder (native/src/seal/c/ckksencoder.h:16-49; seal::CKKSEncoder::encode / decode, native/src/seal/ckks.h:458-789): vectors of
 * N/2 real (Encode1 / Decode1) or complex (Encode2 / Decode2: interleaved re, im) numbers <-> NTT-form plaintexts at a level with a
 * scale.  The double-precision FFT, the rounding and the CRT composition repeat the reference's IEEE operations in its order, so the
 * plaintext words of Encode and the doubles of Decode are the reference's bit for bit (incl. the multi-precision branch for coefficients above 128 bits). */
SHL_FUNC CKKSEncoder_Create(void *context, void **ckks_encoder);
SHL_FUNC CKKSEncoder_Destroy(void *thisptr);
SHL_FUNC CKKSEncoder_SlotCount(void *thisptr, uint64_t *slot_count);
SHL_FUNC CKKSEncoder_Encode1(void *thisptr, uint64_t value_count, double *values, uint64_t *parms_id, double scale, void *destination, void *pool);
SHL_FUNC CKKSEncoder_Encode2(void *thisptr, uint64_t value_count, double *complex_values, uint64_t *parms_id, double scale, void *destination,
                             void *pool);
SHL_FUNC CKKSEncoder_Encode3(void *thisptr, double value, uint64_t *parms_id, double scale, void *destination, void *pool); /* one value in every slot */
SHL_FUNC CKKSEncoder_Encode4(void *thisptr, double value_re, double value_im, uint64_t *parms_id, double scale, void *destination,
                             void *pool); /* one complex value in every slot (c/ckksencoder.h:35) */
SHL_FUNC CKKSEncoder_Encode5(void *thisptr, int64_t value, uint64_t *parms_id, void *destination);
SHL_FUNC CKKSEncoder_Decode1(void *thisptr, void *plain, uint64_t *value_count, double *values, void *pool);
SHL_FUNC CKKSEncoder_Decode2(void *thisptr, void *plain, uint64_t *value_count, double *values, void *pool);
/* Whole batches in device memory (library extensions, like BatchEncoder_*Device).
 * EncodeDevice: device_values = `batch` vectors of value_count <= N/2 doubles ([batch][value_count]) or, is_complex, of
 *   value_count complex numbers ([batch][value_count][2], re and im interleaved as Encode2 takes them); shorter vectors are
 *   zero-padded.  device_words = [batch][K][N] words, K = the number of primes at parms_id: item b equals, word for word, the
 *   reference's encode(values_b, parms_id, scale).data() - the layout Decryptor_DecryptBatch writes for CKKS and
 *   Plaintext_SetFromDevice takes.
 * DecodeDevice: device_words = [batch][K][N] NTT-form words at parms_id (a data level) with `scale`, e.g. Decryptor_DecryptBatch's
 *   output; it is not modified.  device_values = [batch][N/2] doubles (real parts) or, want_complex, [batch][N/2][2]: item b
 *   equals the reference's decode of a plaintext with those words, parms_id and scale, bit for bit.
 * Both run on the NULL stream and return after the work is done (encode synchronises once, at the end); batch == 0 does nothing.
 * Arguments are checked as Encode / Decode and the reference check them (ckks.h:463-509, 686-716) - parms_id, scale,
 * value_count, NULL pointers - and input and output must not overlap: SHL_E_INVALIDARG.  Encode's data-dependent checks (a value
 * that is not finite; a coefficient that is NaN, infinite or too large for the level's modulus, ckks.h:525-548) are made per
 * item on the device: SHL_E_INVALIDARG naming the first failing item, and the output words are then unspecified.  The batch is
 * worked through in chunks whose scratch stays within 256 MiB (one item where an item needs more), returned to the pool. */
SHL_FUNC CKKSEncoder_EncodeDevice(void *thisptr, const double *device_values, uint64_t value_count, uint64_t batch, bool is_complex,
                                  uint64_t *parms_id, double scale, uint64_t *device_words);
SHL_FUNC CKKSEncoder_DecodeDevice(void *thisptr, const uint64_t *device_words, uint64_t batch, uint64_t *parms_id, double scale,
                                  bool want_complex, double *device_values);

/* BatchEncoder (native/src/seal/c/batchencoder.h:16-30; seal::BatchEncoder::encode / decode, native/src/seal/batchencoder.cpp:97-447):
 * N integers modulo t <-> one plaintext polynomial through the NTT modulo t and the matrix index map.  Encode1 / Decode1 take
 * unsigned values, Encode2 / Decode2 signed ones, host vectors as in sealc (Decode writes N values).  The *Device forms convert
 * `batch` vectors [batch][N] that are already in HBM - e.g. the output of Decryptor_DecryptBatch - without leaving it. */
SHL_FUNC BatchEncoder_Create(void *context, void **batch_encoder);
SHL_FUNC BatchEncoder_Destroy(void *thisptr);
SHL_FUNC BatchEncoder_GetSlotCount(void *thisptr, uint64_t *slot_count);
SHL_FUNC BatchEncoder_Encode1(void *thisptr, uint64_t count, uint64_t *values, void *destination);
SHL_FUNC BatchEncoder_Encode2(void *thisptr, uint64_t count, int64_t *values, void *destination);
SHL_FUNC BatchEncoder_Decode1(void *thisptr, void *plain, uint64_t *count, uint64_t *destination, void *pool);
SHL_FUNC BatchEncoder_Decode2(void *thisptr, void *plain, uint64_t *count, int64_t *destination, void *pool);
SHL_FUNC BatchEncoder_EncodeDevice(void *thisptr, const uint64_t *device_values, uint64_t batch, bool is_signed, uint64_t *device_coefficients);
SHL_FUNC BatchEncoder_DecodeDevice(void *thisptr, const uint64_t *device_coefficients, uint64_t batch, bool is_signed, uint64_t *device_values);

/* PublicKey / Encryptor (native/src/seal/c/publickey.h, native/src/seal/c/encryptor.h; seal::Encryptor::encrypt_symmetric / encrypt_zero_symmetric and
 * their Serializable<> forms, native/src/seal/encryptor.cpp:116-330, util/rlwe.cpp:270-395).  The randomness follows the
 * reference: a bootstrap Blake2xb PRNG gives the public seed of c_1 (sample_poly_uniform) and the centred-binomial noise
 * (sample_poly_cbd); c_0 = -(c_1 s + e) [+ plaintext] is computed on the device.  Encryptor_SetSeed installs the reference's seeded
 * factory (every encryption restarts from that 8-word seed: reproducible runs, parity tests); NULL returns to operating-system
 * entropy.  The *Save forms write the SEEDED stream (c_0 + the 64-byte seed of c_1: half the size) a client uploads.
 * Public-key encryption (Encryptor_Encrypt / Encryptor_EncryptZero1; util::encrypt_zero_asymmetric, rlwe.cpp:196-268, then the
 * modulus switch of encryptor.cpp:139-186) draws u from the ternary distribution the way libstdc++'s uniform_int_distribution does
 * (GCC >= 11), which is what makes it byte-identical to a reference built with that library.  PublicKey_Set takes
 * PublicKey::data().data() (2*L*N words); either key of Encryptor_Create may be NULL. */
SHL_FUNC PublicKey_Create(void *context, void **public_key);
SHL_FUNC PublicKey_Destroy(void *thisptr);
SHL_FUNC PublicKey_Set(void *thisptr, const uint64_t *host_words, uint64_t word_count);
SHL_FUNC PublicKey_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC PublicKey_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Encryptor_Create(void *context, void *public_key, void *secret_key, void **encryptor);
SHL_FUNC Encryptor_Encrypt(void *thisptr, void *plaintext, void *destination, void *pool);
SHL_FUNC Encryptor_EncryptZero1(void *thisptr, uint64_t *parms_id, void *destination, void *pool);
SHL_FUNC Encryptor_Destroy(void *thisptr);
/* INSECURE, parity tests only (see KeyGenerator_Create1): every call restarts from this seed.  NULL restores OS entropy. */
SHL_FUNC Encryptor_SetSeed(void *thisptr, const uint64_t *seed);
SHL_FUNC Encryptor_EncryptZero2(void *thisptr, void *destination, void *pool); /* at the first data level (c/encryptor.h:26) */
SHL_FUNC Encryptor_EncryptZeroSymmetric1(void *thisptr, uint64_t *parms_id, bool save_seed, void *destination, void *pool);
SHL_FUNC Encryptor_EncryptZeroSymmetric2(void *thisptr, bool save_seed, void *destination, void *pool); /* c/encryptor.h:34 */
SHL_FUNC Encryptor_EncryptSymmetric(void *thisptr, void *plaintext, bool save_seed, void *destination, void *pool);
SHL_FUNC Encryptor_SymmetricSaveSize(void *thisptr, uint64_t *parms_id, int64_t *result);
SHL_FUNC Encryptor_EncryptZeroSymmetricSave(void *thisptr, uint64_t *parms_id, uint8_t *outptr, uint64_t size, int64_t *out_bytes);
SHL_FUNC Encryptor_EncryptSymmetricSave(void *thisptr, void *plaintext, uint8_t *outptr, uint64_t size, int64_t *out_bytes);
/* Whole batches in device memory (library extensions, like CKKSEncoder_EncodeDevice): `batch` fresh ciphertexts in one call,
 * secret-key (EncryptSymmetricDevice) or public-key (EncryptDevice), without a host round trip per item.
 * device_plain: CKKS - [batch][K][N] NTT-form words at parms_id, the layout CKKSEncoder_EncodeDevice writes and
 *   Decryptor_DecryptBatch returns; `scale` becomes the ciphertext's scale (a normal positive number).  BFV / BGV - [batch][N]
 *   coefficients modulo t, what BatchEncoder_EncodeDevice writes; parms_id must be NULL or the first data level and `scale` is
 *   ignored.  NULL - encrypt zero at parms_id, at every level the per-object EncryptZero* forms accept (scale 1).  A NULL parms_id
 *   means the first data level.  The pointer must be 16-byte aligned (SHL_E_INVALIDARG otherwise).  The words are NOT validated (as with Plaintext_SetFromDevice): CKKS words must be below their
 *   primes and BFV / BGV coefficients below t, or the result is unspecified.
 * destination: a Ciphertext whose batch equals `batch` (SHL_E_INVALIDARG otherwise); it is resized to size 2 at the level and its
 *   is_ntt_form, scale and correction factor (1) are set as the per-object forms set them.  Item b lies where every batch
 *   ciphertext keeps it: word ((p * batch + b) * K + r) * N + j.
 * seeds: host array [batch][8], item b's bootstrap seed.  NULL: with Encryptor_SetSeed installed EVERY item restarts from that
 *   seed (the reference's seeded factory: identical (a, e) in every item - the INSECURE warning of Encryptor_SetSeed applies, as it
 *   does to caller-chosen seeds); otherwise every item draws 64 fresh bytes from the operating system.
 * Item b equals, word for word, what Encryptor_EncryptSymmetric / Encryptor_Encrypt (device_plain NULL: EncryptZeroSymmetric1 /
 * EncryptZero1) give after Encryptor_SetSeed(seeds + 8 b), hence the reference's Encryptor under Blake2xbPRNGFactory(seed_b).
 * Both run on the NULL stream and return when the work is done; batch == 0 does nothing.  Arguments are checked as the per-object
 * forms check them, with their HRESULTs: unknown parms_id, a level the scheme does not encrypt a plaintext at, a destination of
 * another context or batch, device_plain overlapping the destination's words: SHL_E_INVALIDARG; a missing key:
 * SHL_COR_E_INVALIDOPERATION; NULL thisptr / destination: SHL_E_POINTER.  A failed check leaves the destination untouched.  The batch
 * is worked through in chunks of max(1, 256 MiB / (8 K' N)) items, K' = the primes at the level the item is encrypted at (the level
 * above parms_id for the public-key form where there is one), which bounds the scratch of a chunk; it goes back to the pool. */
SHL_FUNC Encryptor_EncryptSymmetricDevice(void *thisptr, const uint64_t *device_plain, uint64_t batch, uint64_t *parms_id, double scale,
                                          const uint64_t *seeds, void *destination);
SHL_FUNC Encryptor_EncryptDevice(void *thisptr, const uint64_t *device_plain, uint64_t batch, uint64_t *parms_id, double scale,
                                 const uint64_t *seeds, void *destination);

/* KSwitchKeys / RelinKeys / GaloisKeys (native/src/seal/c/kswitchkeys.h, relinkeys.h, galoiskeys.h).
 * A key set lives in HBM; one key (index) is uploaded as the concatenation of its decomposition
 * digits, each a size-2 key-level ciphertext in NTT form: [digit][2][L][N] words
 * (KSwitchKeys::keys_[index][digit].data(), native/src/seal/kswitchkeys.h:340). */
/* Plaintext (native/src/seal/c/plaintext.h:16-75; class seal::Plaintext, native/src/seal/plaintext.h), device resident.
 * Coefficient form: `count` coefficients modulo t (BFV/BGV), parms_id = zero.  NTT form: K*N words at a level
 * (Plaintext_Set4 the words, then Plaintext_SetParmsId; CKKS plaintexts are always in this form).  One Plaintext handle is
 * applied to every item of a ciphertext batch; for one plaintext per item see Evaluator_AddPlainDevice / SubPlainDevice /
 * MultiplyPlainDevice, which take the plaintexts as raw device words.  Create1 takes the context where sealc takes a pool handle. */
SHL_FUNC Plaintext_Create1(void *context, void **plaintext);
SHL_FUNC Plaintext_Create5(void *copy, void **plaintext);
SHL_FUNC Plaintext_Destroy(void *thisptr);
SHL_FUNC Plaintext_Set4(void *thisptr, uint64_t count, uint64_t *coeffs);
SHL_FUNC Plaintext_SetFromDevice(void *thisptr, uint64_t count, const uint64_t *device_coeffs);
SHL_FUNC Plaintext_CoeffCount(void *thisptr, uint64_t *coeff_count);
SHL_FUNC Plaintext_IsNTTForm(void *thisptr, bool *is_ntt_form);
SHL_FUNC Plaintext_GetParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC Plaintext_SetParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC Plaintext_Scale(void *thisptr, double *scale);
SHL_FUNC Plaintext_SetScale(void *thisptr, double scale);
SHL_FUNC Plaintext_CopyToHost(void *thisptr, uint64_t *dst, uint64_t word_count); /* synchronises */
/* wire format (native/src/seal/c/plaintext.h:83-89; Plaintext::save / load / unsafe_load, native/src/seal/plaintext.cpp): e.g. the
 * output of CKKSEncoder::encode / BatchEncoder::encode serialized by the client, as Ciphertext_Load above */
SHL_FUNC Plaintext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC Plaintext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
SHL_FUNC Plaintext_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC Plaintext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);

SHL_FUNC KSwitchKeys_Create1(void **kswitch_keys);
SHL_FUNC KSwitchKeys_Destroy(void *thisptr);
SHL_FUNC KSwitchKeys_Size(void *thisptr, uint64_t *size);
SHL_FUNC KSwitchKeys_SetKey(void *thisptr, void *context, uint64_t index, uint64_t digits, const uint64_t *host_words);
SHL_FUNC KSwitchKeys_SetKeyFromDevice(void *thisptr, void *context, uint64_t index, uint64_t digits, const uint64_t *device_words);
/* digit-parallel key switching (section 1b): upload only the decomposition digits [digit_first, digit_first + digits)
 * of key `index` (host_words = those digits, [digits][2][L][N]); this rank then serves exactly that digit range */
SHL_FUNC KSwitchKeys_SetKeyDigits(void *thisptr, void *context, uint64_t index, uint64_t digit_first, uint64_t digits,
                                  const uint64_t *host_words);
SHL_FUNC KSwitchKeys_HasKey(void *thisptr, uint64_t index, bool *has_key);
/* library extension: HBM held by the keys of the object.  At 2^13 <= N <= 2^16 a key is stored in the fused key-switch kernel's
 * register order (pairs of balanced doubles for primes below 2^50, (word, Shoup quotient) pairs for larger ones): 284 MB per C5 key
 * against 252 MB of natural words */
SHL_FUNC KSwitchKeys_DeviceBytes(void *thisptr, uint64_t *bytes);
/* KSwitchKeys::load / unsafe_load (native/src/seal/c/kswitchkeys.h:45-47; kswitchkeys.cpp:92-180): a serialized RelinKeys /
 * GaloisKeys stream (seeded or full, compr_mode none) goes straight into the device key slabs, every key index it holds. */
SHL_FUNC KSwitchKeys_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
/* KSwitchKeys::save_size / save (native/src/seal/c/kswitchkeys.h:41-43; kswitchkeys.cpp:47-90): the FULL keys the object holds, each digit
 * as its size-2 ciphertext stream, byte for byte the reference's stream for compr_mode none (the device words go back from the
 * key-switch kernels' register order to canonical natural order first).  A digit-parallel slice is refused (logic_error). */
SHL_FUNC KSwitchKeys_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC KSwitchKeys_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
SHL_FUNC KSwitchKeys_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
SHL_FUNC RelinKeys_GetIndex(uint64_t key_power, uint64_t *index);
SHL_FUNC GaloisKeys_GetIndex(uint32_t galois_elt, uint64_t *index);
/* GaloisTool::get_elt_from_step (native/src/seal/util/galois.cpp:53-95) */
SHL_FUNC GaloisTool_GetEltFromStep(void *context, int step, uint32_t *galois_elt);

/* Evaluator (native/src/seal/c/evaluator.h).  `destination` may equal `encrypted` (in place). */
SHL_FUNC Evaluator_Create(void *context, void **evaluator);
SHL_FUNC Evaluator_Destroy(void *thisptr);
/* Work of the evaluator is enqueued on `hip_stream` (NULL = the NULL stream), blocking or hipStreamNonBlocking alike.  Device
 * memory recycled through the library's pool is ordered across streams (an event wait when a block changes stream), so
 * several evaluators may run on different streams concurrently.  The destination copy of the out-of-place forms
 * (destination != encrypted) runs on the same stream as the operation.  Three families have no such copy - the result is written
 * straight into `destination` and `encrypted` is only read: Evaluator_Multiply (CKKS 2 x 2 and BFV), and Evaluator_ApplyGalois /
 * RotateRows / RotateColumns / RotateVector / ComplexConjugate when the exact Galois key is present (the reference's
 * "destination = encrypted; op_inplace(destination)", evaluator.h:239-247, 1072-1315, gives the same words).  What differs from
 * the reference is the FAILURE path of these copy-free forms only: the reference has copied the operand into the destination
 * before it validates, so a call that throws leaves a copy of `encrypted` there; here a call that fails its argument checks
 * leaves a separate destination untouched, and a Galois form that fails later (key switch, transparent-ciphertext check) leaves
 * it EMPTY (released) rather than half-built.  The HRESULT and the exception class are the reference's either way. */
SHL_FUNC Evaluator_SetStream(void *thisptr, void *hip_stream);
/* library extension: destination := encrypted, ordered on the evaluator's stream (Ciphertext_Set copies on the calling thread's
 * stream); what a pipeline over several evaluators / streams uses to stage its inputs */
SHL_FUNC Evaluator_CopyTo(void *thisptr, void *encrypted, void *destination);
SHL_FUNC Evaluator_Synchronize(void *thisptr);
/* SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT (evaluator.cpp:386-392) costs a device->host round trip per
 * operation: off by default for device-resident batches, switch on for drop-in error parity. */
SHL_FUNC Evaluator_SetTransparentCheck(void *thisptr, bool enabled);
/* hipGraph capture of a fixed operation sequence (the reference has no counterpart - its operations are host
 * calls).  Between BeginCapture and EndCapture the Evaluator_* operations issued on this evaluator are recorded instead of
 * executed; Evaluator_LaunchGraph replays them with ONE launch, stream-ordered on the evaluator's stream, on the same device
 * buffers: refresh the operand ciphertexts' contents in place (Ciphertext_CopyFromHost/Device, Ciphertext_Load), replay, read the
 * destinations.  Run the sequence once eagerly before capturing; keep the captured objects alive and un-resized; issue the
 * recorded operations from the thread that called BeginCapture.  The scratch blocks the recording used stay reserved for the
 * graph (their addresses are part of it) until Graph_Destroy. */
SHL_FUNC Evaluator_BeginCapture(void *thisptr);
SHL_FUNC Evaluator_EndCapture(void *thisptr, void **graph);
SHL_FUNC Evaluator_LaunchGraph(void *thisptr, void *graph);
SHL_FUNC Graph_Destroy(void *graph);
SHL_FUNC Evaluator_Negate(void *thisptr, void *encrypted, void *destination);
SHL_FUNC Evaluator_Add(void *thisptr, void *encrypted1, void *encrypted2, void *destination);
SHL_FUNC Evaluator_Sub(void *thisptr, void *encrypted1, void *encrypted2, void *destination);
SHL_FUNC Evaluator_Multiply(void *thisptr, void *encrypted1, void *encrypted2, void *destination, void *pool);
/* plaintext operands and many-operand forms (native/src/seal/c/evaluator.h:24-37, 47-49, 59-64;
 * Evaluator::add_many / add_plain / sub_plain / multiply_plain / multiply_many / exponentiate /
 * transform_to_ntt(Plaintext) / mod_switch_to[_next](Plaintext), native/src/seal/evaluator.cpp:242-261, 1369-1402, 1649-2287) */
SHL_FUNC Evaluator_AddMany(void *thisptr, uint64_t count, void **encrypteds, void *destination);
SHL_FUNC Evaluator_AddPlain(void *thisptr, void *encrypted, void *plain, void *destination);
SHL_FUNC Evaluator_SubPlain(void *thisptr, void *encrypted, void *plain, void *destination);
SHL_FUNC Evaluator_MultiplyMany(void *thisptr, uint64_t count, void **encrypteds, void *relin_keys, void *destination, void *pool);
SHL_FUNC Evaluator_MultiplyPlain(void *thisptr, void *encrypted, void *plain, void *destination, void *pool);
SHL_FUNC Evaluator_Exponentiate(void *thisptr, void *encrypted, uint64_t exponent, void *relin_keys, void *destination, void *pool);
SHL_FUNC Evaluator_TransformToNTT1(void *thisptr, void *plain, uint64_t *parms_id, void *destination_ntt, void *pool);
SHL_FUNC Evaluator_ModSwitchToNext2(void *thisptr, void *plain, void *destination);
SHL_FUNC Evaluator_ModSwitchTo2(void *thisptr, void *plain, uint64_t *parms_id, void *destination);
/* One plaintext PER ITEM of a device-resident batch (library extensions, like Encryptor_EncryptDevice): plaintext b is applied to
 * item b of `encrypted`, where a Plaintext handle is applied to every item.
 * device_plain: `batch` plaintexts in device memory, 16-byte aligned, batch == the ciphertext's batch.
 *   plain_is_ntt false - [batch][N] coefficients modulo t, what BatchEncoder_EncodeDevice writes (BFV / BGV only);
 *   plain_is_ntt true  - [batch][K][N] NTT-form words at the ciphertext's own level, what CKKSEncoder_EncodeDevice and
 *                        Evaluator_TransformPlainToNTTDevice write (CKKS plaintexts are always in this form).
 *   The words are NOT validated (as with Plaintext_SetFromDevice): out of range, the result is unspecified.
 * scale: the plaintexts' common scale for CKKS (a normal positive number): AddPlainDevice / SubPlainDevice require it to be close
 *   to the ciphertext's, MultiplyPlainDevice multiplies the scales and checks the bound.  Ignored for BFV / BGV.
 * Item b of the result equals, word for word, Evaluator_AddPlain / SubPlain / MultiplyPlain on a batch of one with a Plaintext that
 * holds item b's words, hence the reference's add_plain_inplace / sub_plain_inplace / multiply_plain_inplace; is_ntt_form, scale and
 * correction factor of the result are what those leave.  The accepted combinations of forms are theirs too: CKKS NTT x NTT; BFV
 * add / sub coefficient x coefficient; BGV add / sub NTT ciphertext x coefficient plaintext (the plaintext is multiplied by the
 * ciphertext's correction factor modulo t before the lift); multiply every combination of forms except a coefficient-form
 * plaintext for CKKS.  A coefficient-form ciphertext times coefficient-form plaintexts reproduces the reference's monomial branch
 * PER ITEM (a plaintext with one non-zero coefficient is multiplied in as the raw coefficient under the fast plain lift; a batch
 * may mix such items with others): all items are decided by one statistics kernel and ONE read-back, so this combination
 * synchronises the evaluator's stream once and cannot be recorded by Evaluator_BeginCapture, exactly like the per-object form; every
 * other combination is enqueued without a host round trip and records.
 * destination == encrypted works in place.  Otherwise `encrypted` is only read and the result is written straight into
 * `destination`, which takes the ciphertext's shape and metadata (no copy of the operand first); a call that fails its argument
 * checks leaves it untouched.  Checks and HRESULTs are those of the per-object forms (invalid ciphertext, wrong form for the
 * scheme, scale mismatch / out of bounds: SHL_E_INVALIDARG; NULL handles: SHL_E_POINTER), and SHL_E_INVALIDARG for: batch == 0 or
 * != the ciphertext's batch, a NULL or misaligned device_plain, device_plain overlapping the words of `encrypted` or `destination`.
 * With Evaluator_SetTransparentCheck on, the result is checked over the whole batch.
 * The lifted plaintexts of a BFV / BGV call ([batch][K][N] words) are scratch: the batch is worked through in chunks of
 * max(1, 256 MiB / (8 K N)) items and the scratch goes back to the pool. */
SHL_FUNC Evaluator_AddPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt,
                                  double scale, void *destination);
SHL_FUNC Evaluator_SubPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt,
                                  double scale, void *destination);
SHL_FUNC Evaluator_MultiplyPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt,
                                       double scale, void *destination);
/* [batch][N] coefficients modulo t -> [batch][K][N] NTT-form words at parms_id, item for item Evaluator_TransformToNTT1 (centred
 * lift, forward transform): plaintexts that are used many times are lifted and transformed once and then passed with
 * plain_is_ntt = true.  BFV / BGV; CKKS is refused as the per-object form refuses it.  SHL_E_INVALIDARG for an unknown parms_id,
 * batch == 0, a NULL or misaligned (16 bytes) device pointer, input overlapping output.  Enqueued on the evaluator's stream. */
SHL_FUNC Evaluator_TransformPlainToNTTDevice(void *thisptr, const uint64_t *device_coefficients, uint64_t batch, uint64_t *parms_id,
                                             uint64_t *device_words);
/* Sums over the ITEMS of a device-resident batch (library extensions): the one thing the per-item forms above do not do is combine
 * items - the aggregation sum_b ct_b, its weighted form, and the encrypted matrix-vector / database dot product
 * sum_b ct_b (.) pt_b with one plaintext per row, optionally in groups of rows.
 * encrypted: a batch of B items, any size >= 2, at any level.  group = g >= 1 must divide B.  destination: ANOTHER handle whose batch
 * is B / g, made with Ciphertext_CreateBatch (the convention of Encryptor_EncryptDevice's destination); it is resized to the operand's
 * size and level.  Output item o is the sum over the input items o g .. o g + g - 1: g = B gives one ciphertext; g = 1 is a copy for
 * SumItems and the words of MultiplyPlainDevice for DotPlainDevice.  `encrypted` is only read.
 * Evaluator_SumItems: item o equals, word for word, Evaluator_AddMany over batch-of-one ciphertexts holding those items, hence the
 *   reference's add_many (evaluator.cpp:242-261).  Every form and scheme Evaluator_Add accepts; the items of a batch share scale and
 *   correction factor, so the reference's CKKS scale check and BGV correction-factor branch are the equal case.  is_ntt_form, scale
 *   and correction factor of the result are the operand's.
 * Evaluator_DotPlainDevice: device_plain = [B][K][N] NTT-form words at the ciphertext's level (what CKKSEncoder_EncodeDevice and
 *   Evaluator_TransformPlainToNTTDevice write), 16-byte aligned, batch == B, NOT validated like the other *Device forms.  The
 *   ciphertext must be in NTT form: CKKS, BGV, or BFV after Evaluator_TransformToNTT2.  Item o equals Evaluator_MultiplyPlainDevice
 *   with plain_is_ntt = true followed by the sum above, hence the reference's multiply_plain_inplace (evaluator.cpp:2157-2194) per
 *   item and then add_many; scale handling (CKKS: the scales are multiplied), the scale-bound check and the metadata are those of
 *   that composition.  Coefficient-form plaintexts are deliberately NOT accepted - run Evaluator_TransformPlainToNTTDevice first:
 *   the coefficient x coefficient monomial branch of the product is per item and data dependent and has no place in a reduction.
 * SHL_E_POINTER: NULL handles.  SHL_E_INVALIDARG: an invalid ciphertext; g == 0 or g does not divide B; batch != B; the destination's
 * batch != B / g; destination == encrypted; a NULL or misaligned device_plain; device_plain overlapping the words of `encrypted` or
 * `destination`; a ciphertext in coefficient form (DotPlainDevice); a scale out of bounds.  A failed check leaves the destination
 * untouched.  With Evaluator_SetTransparentCheck on, the result batch is checked.
 * Both calls are enqueued on the evaluator's stream without a host round trip and record under Evaluator_BeginCapture.  Terms are
 * accumulated as plain integers and reduced once per 16 (sums) / 256 (products) of them: with primes below 2^60 that many fit 64 /
 * 128 bits.  A small result (fewer than 2^17 output pairs, at least 8 items per group) is computed in up to 64 slices of the group
 * by separate workgroups into pool scratch of slices x one result batch, which a second launch adds; the words do not depend on it. */
SHL_FUNC Evaluator_SumItems(void *thisptr, void *encrypted, uint64_t group, void *destination);
SHL_FUNC Evaluator_DotPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, uint64_t group, double scale,
                                  void *destination);
/* The ciphertext x ciphertext reduction over the ITEMS of two device-resident batches (library extension): sum_b x_b (x) y_b - an
 * encrypted inner product, an encrypted matrix times an encrypted vector with one ciphertext per row or column, a squared distance
 * sum_b (x_b)^2.  The sum is formed BEFORE relinearising (relinearisation is linear): one Evaluator_Relinearize on the result serves a
 * whole group.  No product is stored: each operand word crosses HBM once and the result is written once.
 * encrypted1, encrypted2: batches of B items, CKKS or BGV, both of size 2, in NTT form, at the same level; they may be the same
 * handle (the sum of squares; the operand is then read once).  group = g >= 1 must divide B.  destination: ANOTHER handle whose batch
 * is B / g, made with Ciphertext_CreateBatch, different from both operands; it is resized to size 3 at the operands' level.
 * Output item o equals, word for word, Evaluator_Multiply on batches of one holding the items o g .. o g + g - 1 followed by
 * Evaluator_AddMany over the products, hence the reference's multiply (evaluator.cpp ckks_multiply / bgv_multiply) and then add_many.
 * g = 1 gives exactly Evaluator_Multiply's words.  is_ntt_form is true; CKKS: scale = scale1 * scale2 with the reference's
 * scale-bound check; BGV: correction factor = cf1 * cf2 mod t (the items of a batch share it, so the sum is the equal-factor case);
 * parms_id is the operands'.
 * BFV is refused (SHL_E_INVALIDARG, "unsupported scheme"): its product rounds per item (BEHZ), sum_b round(.) is not round(sum_b .),
 * so a fused form could not give the reference's words.  Sizes other than 2 x 2 are refused with SHL_E_INVALIDARG: the sum is taken
 * before relinearising, on fresh or relinearised operands, and those have size 2.
 * SHL_E_POINTER: NULL handles.  SHL_E_INVALIDARG: an invalid ciphertext; mismatched levels or batches; a ciphertext in coefficient
 * form; g == 0 or g does not divide B; the destination's batch != B / g; destination == an operand; a scale out of bounds.  A failed
 * check leaves the destination untouched.  With Evaluator_SetTransparentCheck on, the result batch is checked.
 * Operands with a deferred key-switch tail or a deferred product pending are settled before they are read; the result is stored at
 * once (never a deferred product).  Enqueued on the evaluator's stream without a host round trip; records under
 * Evaluator_BeginCapture.  Products are accumulated as plain 128-bit integers and reduced once per 128 items (the middle polynomial
 * adds two products per item, and 256 products of words below 2^60 fit 128 bits).  A small result is computed in slices by the rule
 * of Evaluator_SumItems, with pool scratch of slices x 3 x one result plane. */
SHL_FUNC Evaluator_DotItems(void *thisptr, void *encrypted1, void *encrypted2, uint64_t group, void *destination);
/* Item maps (library extensions): the three reductions above over the items a device-resident CSR list names, instead of over
 * consecutive groups - select, repeat, permute or compact the items of a batch on the device (a gather), sum groups of unequal length
 * (aggregation by bucket, federated sums with drop-outs), multiply a sparse plaintext matrix with a vector of ciphertexts (row o
 * adds the few items its non-zeros name), or sum x_i (x) y_j over a list of pairs (i, j).
 * ItemMap_Create: row_offsets is a host array of rows + 1 entries, first_items and second_items host arrays of
 *   terms = row_offsets[rows] entries.  Term t of row o (row_offsets[o] <= t < row_offsets[o + 1]) names item first_items[t] of the
 *   first operand and second_items[t] of the second; second_items == NULL means "the same list", and second_batch must then equal
 *   first_batch.  Everything is validated once, here, with SHL_E_INVALIDARG: rows >= 1; row_offsets[0] == 0 and strictly increasing (an
 *   empty row would be a transparent ciphertext, and add_many of nothing throws in the reference); rows and terms below 2^32; every
 *   item number below its batch; NULL arrays.  The lists are uploaded once, as 32-bit words, each 16-byte aligned, with a plain
 *   synchronous copy after draining the device: this is not a hot-path call.  The calls below read them from HBM and make no host
 *   transfer, so they record under Evaluator_BeginCapture and one map serves many calls (a fixed sparse matrix).
 * ItemMap_Destroy gives the lists back through the stream-aware device pool and drains nothing: a block that work may still read is
 *   not handed to another user before that user has waited for every stream registered with the pool and for the NULL stream, so a
 *   map may be destroyed right after the call that used it - but not before the last launch of a graph that recorded it.
 * ItemMap_Info: any of the outputs may be NULL.
 * The three calls: the output is a batch of `rows` items; destination is ANOTHER handle made with Ciphertext_CreateBatch(rows),
 * distinct from every operand.
 * Evaluator_SumItemsMapped: item o = sum_t ct[first[t]].  Only the first list is used; every size, form and scheme Evaluator_SumItems
 *   accepts; encrypted's batch must equal first_batch.  A map whose rows all have one term is a gather: the words are copied exactly,
 *   because the canonical residue of one canonical word is that word.
 * Evaluator_DotPlainMapped: item o = sum_t ct[first[t]] (.) pt[second[t]].  device_plain = [plain_count][K][N] NTT-form words at the
 *   ciphertext's level, plain_count == second_batch, which may differ from the ciphertext's batch (weights per non-zero, or weights
 *   shared per column).  The ciphertext is in NTT form; scale, alignment, overlap and "NOT validated" exactly as
 *   Evaluator_DotPlainDevice.
 * Evaluator_DotItemsMapped: item o = sum_t x[first[t]] (x) y[second[t]], size 3, not relinearised.  CKKS / BGV, size 2 x 2, NTT form,
 *   the same level; BFV is refused as Evaluator_DotItems refuses it.  x's batch must equal first_batch and y's second_batch; the two
 *   may differ.  The square kernel (x read once) applies when encrypted1 == encrypted2 and the map has no second list.
 * Output item o equals, word for word, the per-object forms on batches of one holding the named items followed by Evaluator_AddMany,
 * hence the reference's multiply_plain_inplace / multiply and then add_many: a modular sum does not depend on which items it is told
 * to add.  An item named twice is added twice.  Metadata (scale product and its bound check, correction factor, is_ntt_form,
 * parms_id), the settle-before-read rules for operands with a deferred tail or a pending product, Evaluator_SetTransparentCheck and
 * "a failed check leaves the destination untouched" are those of the contiguous forms, and so are their SHL_E_POINTER /
 * SHL_E_INVALIDARG cases, with these instead of the group's: an operand's batch != the map's, plain_count != second_batch, the
 * destination's batch != rows, a map of another context.
 * The calls are enqueued on the evaluator's stream without a host round trip.  The kernels are those of the contiguous forms with
 * another walk: from N = 128 on a wavefront never leaves its row and reads offsets and item numbers through the scalar cache, one
 * 4-byte load per wavefront, list and term; on smaller rings every lane reads its own.  A small result is cut as for
 * Evaluator_SumItems: WHETHER to cut, and into how many slices, follows from the mean row - that rule asked with
 * ceil(terms / rows) items per group; the slices are then sized from the longest row, per_slice = ceil(longest_row / slices), and
 * ceil(longest_row / per_slice) of them run.  Slice s of row o adds the terms [off[o] + s per_slice, min(off[o + 1], off[o] + (s + 1)
 * per_slice)) and writes zeros where that is empty; the words do not depend on it.  A very skewed map (one long row among short
 * ones) is balanced by this cut and by nothing else. */
SHL_FUNC ItemMap_Create(void *context, uint64_t rows, const uint64_t *row_offsets, const uint64_t *first_items, const uint64_t *second_items,
                        uint64_t first_batch, uint64_t second_batch, void **item_map);
SHL_FUNC ItemMap_Destroy(void *thisptr);
SHL_FUNC ItemMap_Info(void *thisptr, uint64_t *rows, uint64_t *terms, uint64_t *longest_row, uint64_t *first_batch, uint64_t *second_batch);
SHL_FUNC Evaluator_SumItemsMapped(void *thisptr, void *encrypted, void *item_map, void *destination);
SHL_FUNC Evaluator_DotPlainMapped(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t plain_count, void *item_map,
                                  double scale, void *destination);
SHL_FUNC Evaluator_DotItemsMapped(void *thisptr, void *encrypted1, void *encrypted2, void *item_map, void *destination);
/* Galois sets - many rotations of a batch in one key switch (GaloisSet_Create, Evaluator_ApplyGaloisSet) - are declared in
 * sealhip_galois_set.h, which this header includes at its end. */
/* A sparse matrix of SCALAR weights over an item map (library extension): Evaluator_DotPlainMapped whose plaintexts are constants,
 *   out_o = sum_{t in row o} const(w[second[t]]) (.) ct[first[t]],   row_offsets[o] <= t < row_offsets[o + 1],  o < rows
 * - with one ciphertext per feature and the samples in the slots: a pruned dense layer, grouped, depthwise and dilated convolutions,
 * average pooling with any window, transposed and 1-D convolution, graph aggregation with edge weights, banded operators.  A weight
 * is [K] words or one integer where Evaluator_DotPlainMapped needs [K][N] words (N = 65536, K = 15: 7.9 MB per weight).
 * encrypted = a batch of first_batch items, any size >= 2, any level, in NTT form (CKKS, BGV, or BFV after
 *   Evaluator_TransformToNTT2); destination = ANOTHER handle made with Ciphertext_CreateBatch(rows), resized to the operand's size
 *   and level; weight_count must equal the map's second_batch, so a map made without a second list means one weight per input
 *   item.  An item or a weight named twice is used twice.  One map and one weight buffer serve many calls.
 * flags: bit 2 clear = WIDE weights, [weight_count][K] 64-bit words at the ciphertext's level, as the three scalar producers write
 *   them; bit 2 set = NARROW weights, [weight_count] signed 32-bit integers.  The meaning of each form, of `scale`, the 16-byte
 *   alignment, "not validated" and THE WEIGHTS MUST HAVE BEEN WRITTEN BY SOMETHING EARLIER ON THE STREAM are exactly
 *   Evaluator_MatMulScalarsItems' (below), whose bit this is.  Every other bit, bits 0 and 1 included, is SHL_E_INVALIDARG.
 * Contract: output item o equals, word for word and in its metadata, Evaluator_DotPlainMapped with the same map on
 *   [weight_count][K][N] plaintexts each filled with its weight's K words, hence the reference's multiply_plain_inplace per term
 *   followed by add_many.  The narrow form's words are the wide form's on the words its weights stand for.  Over the dense map (row
 *   o names the items 0 .. B - 1, term (o, b) names weight o B + b) the words are Evaluator_DotScalarsDevice's; over the map of the
 *   in-image taps with weight o * inner + tap they are Evaluator_Conv2dScalarsItems'.  Metadata (scale product and its bound check,
 *   correction factor, is_ntt_form, parms_id), the settle-before-read of an operand with a deferred tail or a pending product,
 *   Evaluator_SetTransparentCheck on the result batch and "a failed check leaves the destination untouched" are
 *   Evaluator_DotPlainMapped's.  SHL_E_POINTER for NULL handles.  SHL_E_INVALIDARG: an unknown flag bit; weight_count !=
 *   second_batch; the ciphertext's batch != first_batch; the destination's batch != rows; destination == encrypted; NULL or
 *   misaligned device_weights; weights overlapping the words of either ciphertext; a coefficient-form ciphertext; an invalid or
 *   foreign ciphertext, or a map of another context; a scale out of bounds.  The kernel indexes the weights in 64 bits, so
 *   weight_count * K has no bound of its own (weight_count is a second_batch, below 2^32).
 * The call is enqueued on the evaluator's stream without a host round trip and records under Evaluator_BeginCapture.
 * Kernel: the mapped reductions' with one more term.  One thread holds one 16-byte coefficient pair of one prime, one plane and
 *   one output item (the planes are in the grid: the weight is a scalar, so nothing is gained by holding it over the planes).  From
 *   N = 128 on a wavefront never leaves its row and a term is a chain of scalar loads through the constant cache - the two list
 *   entries, then the weight - and one vector load; four terms are in flight per wavefront (the list entries of four consecutive
 *   terms are one 16-byte scalar load each).  On smaller rings every lane reads its own.  Wide products are accumulated as 128-bit
 *   integers and reduced once per 256 terms; narrow ones use the biased weight and the two exact sums of
 *   Evaluator_MatMulScalarsItems, reduced once per 1024 terms.
 * Cut: the mapped family's (above), the rule being asked with size rows K N / 2 threads: WHETHER to cut, and into how many slices,
 *   follows from the mean row; the slices are sized from the longest row, slices past the end of a short row store zeros, and a
 *   second launch adds the slices from pool scratch [slices][size][rows][K][N].  The words do not depend on the cut.
 * Bytes: at size 2 a term and coefficient pair reads two ciphertext pairs (32 B) where Evaluator_DotPlainMapped reads those and a
 *   plaintext pair (48 B): 1.5 x fewer.  Measured on one MI355X (CKKS, size 2, both forms alike, against the DotPlainMapped kernel
 *   over the same map on expanded plaintexts; DESIGN.md 8.12 has the table): at N = 65536, K = 15, 1.59 x for a pruned layer of 64
 *   rows x 8 terms (1.51 ms), 1.57 x for a depthwise 3 x 3 over 8 channels of 8 x 8 (11.3 ms), 1.48 x for the dense 16 x 64 map
 *   (2.72 ms) and 1.24 x for 2 x 2 pooling, whose rows have 4 terms; 6.0 - 6.3 TB/s by this model and 0.63 - 0.74 Tmac/s: bound by
 *   HBM, not by the scalar-load chain.  At N = 8192, K = 3, where the operands come from the caches: 1.09 x (pooling) to 2.1 x
 *   (dense).  Where the map IS dense, Evaluator_DotScalarsDevice reads the operand once per four rows and is 3.1 x faster than this
 *   call at N = 65536.  Not measured: other sizes, rings below N = 8192 (so none of the per-lane kernels), BGV / BFV. */
SHL_FUNC Evaluator_DotScalarsMapped(void *thisptr, void *encrypted, const void *device_weights, uint64_t weight_count, void *item_map,
                                    uint64_t flags, double scale, void *destination);
/* Scalar weights (library extensions): a dense plaintext matrix of SCALARS times a vector of ciphertexts,
 * out_o = sum_b w[o][b] * ct_b - the encrypted linear layer with one ciphertext per feature and the samples in the slots, weighted
 * averaging, any change of basis over the items.  A plaintext that holds one value in every slot is a constant polynomial, and in
 * NTT form it is the same word at all N positions of a prime: a scalar at a level with K primes is K words, word k being the value
 * every coefficient of prime k holds.  Scalars are [count][K] words in device memory; three host-side producers make them, each
 * host array in, caller's device buffer out.  They are not hot-path calls: the words are computed on the host and uploaded with one
 * synchronous copy after draining the device, as ItemMap_Create uploads its lists.
 * CKKSEncoder_EncodeScalars: scalar i equals, word for word, what CKKSEncoder_Encode3(values[i], parms_id, scale) puts at every
 *   coefficient, in all three branches of the reference (ckks.cpp:145-226: values of at most 64 bits, at most 128 bits, and the
 *   multi-precision one).  Checks and messages are Encode3's - a scale out of bounds, a value that is not finite or too large - and
 *   name the first failing index; a failed call writes nothing.  The values are host doubles on purpose: the reference's branch and
 *   range checks go through log2 of the host libm.
 * CKKSEncoder_EncodeIntegerScalars: the same against CKKSEncoder_Encode5 (scale 1.0).
 * Evaluator_LiftScalars (BFV / BGV): scalar i equals what Evaluator_TransformPlainToNTTDevice leaves at every coefficient for the
 *   polynomial values_mod_t[i] * X^0 - the centred lift of the reference's transform_to_ntt_inplace(Plaintext) in both its branches
 *   (with and without the fast plain lift); the forward transform of a constant is that constant.  Values >= t are refused, CKKS is
 *   refused as TransformPlainToNTTDevice refuses it.
 * All three: SHL_E_INVALIDARG for an unknown parms_id, count == 0, NULL arrays and a device pointer that is not 16-byte aligned;
 * SHL_E_POINTER for a NULL handle (LiftScalars: or a NULL parms_id).
 * Evaluator_DotScalarsDevice: encrypted = a batch of B items, any size >= 2, any level, in NTT form (CKKS, BGV, or BFV after
 *   Evaluator_TransformToNTT2); device_scalars = [rows][B][K] words at the ciphertext's level, 16-byte aligned, batch == B, NOT
 *   validated like every *Device plaintext (out-of-range words give an unspecified result); destination = ANOTHER handle made with
 *   Ciphertext_CreateBatch(rows), resized to the operand's size and level.  Output item o = sum_b ct_b (.) const(s[o][b]): word for
 *   word Evaluator_DotPlainMapped with the dense map (row o names the items 0 .. B - 1, term (o, b) names plaintext o B + b) and
 *   [rows B][K][N] plaintexts each filled with its scalar's K words, hence the reference's multiply_plain_inplace with the encoded
 *   scalar per item and then add_many.  `scale` is the scalars' common scale (CKKS).  Metadata (scale product and its bound check,
 *   correction factor, is_ntt_form, parms_id), the settle-before-read of an operand with a deferred tail or a pending product,
 *   Evaluator_SetTransparentCheck on the result batch, "a failed check leaves the destination untouched" and the SHL_E_POINTER cases
 *   are those of Evaluator_DotPlainDevice.  SHL_E_INVALIDARG in addition: rows == 0; rows B >= 2^32; batch != B; the destination's
 *   batch != rows; destination == encrypted; scalars overlapping either ciphertext's words; a coefficient-form ciphertext.  A zero
 *   scalar is an ordinary word: only the result batch is subject to the transparent check.  The sparse form is Evaluator_DotScalarsMapped.
 *   The call is enqueued on the evaluator's stream without a host round trip and records under Evaluator_BeginCapture.  One thread
 *   holds one 16-byte coefficient pair of one plane and prime for a tile of 4 consecutive output rows and uses each loaded ciphertext
 *   pair for all of them, so the operand is read once per tile of rows (ceil(rows / 4) size P bytes for an operand plane of P bytes,
 *   against (size + 1) rows P through the dense map), and needs [rows][B][K] words of weights instead of [rows B][K][N].  From
 *   N = 128 on a wavefront never leaves its row and reads the weights with scalar loads through the constant cache: THE SCALARS MUST
 *   HAVE BEEN WRITTEN BY SOMETHING EARLIER ON THE STREAM (a copy, one of the producers above, a previous kernel), like the lists of
 *   an item map.  Products are accumulated as plain 128-bit integers and reduced once per 256 items.  A small result is cut as for
 *   Evaluator_DotPlainDevice, the rule being asked with size ceil(rows / 4) K N / 2 threads that each add B terms; slices of B are
 *   computed by separate workgroups into pool scratch [slices][size][rows][K][N], which a second launch adds; the words do not
 *   depend on it. */
SHL_FUNC CKKSEncoder_EncodeScalars(void *thisptr, uint64_t count, const double *values, uint64_t *parms_id, double scale, uint64_t *device_words);
SHL_FUNC CKKSEncoder_EncodeIntegerScalars(void *thisptr, uint64_t count, const int64_t *values, uint64_t *parms_id, uint64_t *device_words);
SHL_FUNC Evaluator_LiftScalars(void *thisptr, uint64_t count, const uint64_t *values_mod_t, uint64_t *parms_id, uint64_t *device_words);
SHL_FUNC Evaluator_DotScalarsDevice(void *thisptr, void *encrypted, const uint64_t *device_scalars, uint64_t rows, uint64_t batch, double scale,
                                    void *destination);
/* Ciphertext matrix times ciphertext matrix (library extension): out[i][j] = sum_k X[i][k] (x) Y[k][j] with one ciphertext per
 * entry and the samples in the slots - Q K^T, a Gram or covariance matrix X X^T, all pairwise inner products or squared distances
 * between two sets of encrypted vectors.  encrypted1 = a batch of rows * inner items, item (i, k) at i * inner + k; encrypted2 = a
 * batch of inner * cols items, item (k, j) at k * cols + j, or - flags bit 0 - stored [cols][inner] with item (k, j) at j * inner + k;
 * any other bit of flags is SHL_E_INVALIDARG.  CKKS or BGV, both operands of size 2, in NTT form and at the same level; BFV is
 * refused with "unsupported scheme" as Evaluator_DotItems refuses it, and other sizes are refused.  The operands may be the same
 * handle (X X^T with flags = 1 and rows == cols; no symmetric shortcut is taken).  destination = ANOTHER handle made with
 * Ciphertext_CreateBatch(rows * cols), distinct from both operands, resized to size 3 at the operands' level; item (i, j) is at
 * i * cols + j.  It is not relinearised and never a deferred product.
 * Contract: output item (i, j) equals, word for word, Evaluator_DotItemsMapped over the map whose row i * cols + j names the pairs
 * (i * inner + k, k * cols + j) for k < inner, hence the reference's multiply per pair and then add_many.  rows = cols = 1 gives
 * Evaluator_DotItems' words with group = inner; inner = 1 gives Evaluator_Multiply's words for every pair.
 * Metadata (the scale product with the reference's bound check, the correction-factor product mod t, is_ntt_form = true, the
 * operands' parms_id), the settle-before-read of operands with a deferred tail or a pending product, Evaluator_SetTransparentCheck
 * on the result batch and "a failed check leaves the destination untouched" are Evaluator_DotItems'.  SHL_E_POINTER for a NULL
 * handle.  SHL_E_INVALIDARG: rows, inner or cols == 0; rows * inner, inner * cols or rows * cols >= 2^32; encrypted1's batch !=
 * rows * inner or encrypted2's != inner * cols; the destination's batch != rows * cols; the destination is an operand; a
 * coefficient-form operand; mismatched levels; a scale out of bounds; a result too large for one launch (the rows of the flat grid
 * are numbered in 32 bits).  The call is enqueued on the evaluator's stream without a host round trip and records under
 * Evaluator_BeginCapture.
 * One thread holds a tile of 2 consecutive output rows x 4 consecutive output columns of one coefficient position of one prime: per
 * k it loads the 2 x-items and 4 y-items once, both planes each, with the non-temporal hint, and uses them for all 8 outputs - 1.5
 * plane-items read per term (i, j, k) where the mapped route reads 4.  Partial tiles at the right and bottom edges read and write
 * nothing outside the batches.  Products are accumulated as plain 128-bit integers and reduced once per 128 values of k.  A small
 * result is cut as for Evaluator_DotItems, the rule being asked with ceil(rows / 2) ceil(cols / 4) K N threads that each add `inner`
 * terms: slices of the inner index are computed by separate workgroups into pool scratch [slices][3][rows cols][K][N], which a
 * second launch adds; the words do not depend on it.  Measured on one MI355X (profiles/matmul_items.txt): 2.3 - 2.5 times the mapped
 * route at N = 65536, K = 15 from 4 x 16 x 4 on; slower than it at rows = cols = 1 (use Evaluator_DotItems) and at N = 8192, 4 x 16 x 4. */
SHL_FUNC Evaluator_MatMulItems(void *thisptr, void *encrypted1, void *encrypted2, uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags,
                               void *destination);
/* Plaintext matrix times ciphertext matrix (library extension): out[i][j] = sum_k P[i][k] (.) X[k][j] with one full plaintext and
 * one ciphertext per entry and the samples in the slots - packed (per-slot) weights applied to encrypted activations, the giant
 * step sum_k diag_k (.) rot_k(x) of a diagonal-method product for many right-hand sides, a block-sparse layer one dense block at a
 * time.  device_plain = [rows * inner][K][N] NTT-form words at the ciphertext's level, plaintext (i, k) at i * inner + k - what
 * CKKSEncoder_EncodeDevice and Evaluator_TransformPlainToNTTDevice write -, 16-byte aligned and NOT validated, as for
 * Evaluator_DotPlainDevice; coefficient-form plaintexts are not taken.  encrypted = a batch of inner * cols items, item (k, j) at
 * k * cols + j, of any size >= 2 at any level in NTT form: CKKS, BGV, or BFV after Evaluator_TransformToNTT2 (a plaintext product
 * does not round).  destination = ANOTHER handle made with Ciphertext_CreateBatch(rows * cols), resized to the operand's size and
 * level; item (i, j) is at i * cols + j.  `scale` is the plaintexts' (CKKS; ignored otherwise).
 * flags bit 0: the ciphertext matrix is stored [cols][inner], item (k, j) at j * inner + k.  Bit 1: the RESULT is stored
 * [cols][rows], item (i, j) at j * rows + i.  Any other bit is SHL_E_INVALIDARG.  The plaintexts need no flag: the caller encodes
 * them in whatever order it likes.  With both bits set, X W with the ciphertexts on the left is this call on the transposes with no
 * data movement: (X W)[a][b] = sum_k W^T[b][k] X^T[k][a], so rows = W's columns, cols = X's rows, X as it is stored is X^T stored
 * [cols][inner], and the result comes out as X W stored [X's rows][W's columns].
 * Contract: output item (i, j) equals, word for word and in its metadata, Evaluator_DotPlainMapped over the dense map whose row
 * i * cols + j names, for k < inner, ciphertext item k * cols + j and plaintext i * inner + k - hence the reference's
 * multiply_plain_inplace per pair and then add_many.  rows = cols = 1 gives Evaluator_DotPlainDevice's words with group = inner;
 * inner = 1 gives Evaluator_MultiplyPlainDevice's words (plain_is_ntt = true) on the corresponding pairs.  Bit 1 permutes items
 * and nothing else.
 * Metadata (the scale product with the reference's bound check, the correction factor, is_ntt_form and parms_id), the
 * settle-before-read of an operand with a deferred key-switch tail or a pending product, Evaluator_SetTransparentCheck on the
 * result batch and "a failed check leaves the destination untouched" are Evaluator_DotPlainDevice's.  SHL_E_POINTER for a NULL
 * handle.  SHL_E_INVALIDARG: rows, inner or cols == 0; rows * inner, inner * cols or rows * cols >= 2^32; the ciphertext's batch
 * != inner * cols; the destination's batch != rows * cols; destination == encrypted; a NULL or misaligned device_plain;
 * device_plain overlapping the words of either ciphertext; a coefficient-form ciphertext; an invalid or foreign ciphertext; a
 * scale out of bounds; a result too large for one launch (the rows of the flat grid are numbered in 32 bits).  The call is
 * enqueued on the evaluator's stream without a host round trip and records under Evaluator_BeginCapture.
 * One thread holds a tile of 4 consecutive output rows x 4 consecutive output columns of one coefficient position of one prime
 * and one plane (the planes are in the grid): per k it loads the 4 plaintext words and the 4 ciphertext words once and uses them
 * for all 16 products - 0.5 plane-items read per term and plane where the mapped route reads (size + 1) / size.  Partial tiles
 * at the right and bottom edges read and write nothing outside the operands.  Products are accumulated as plain 128-bit integers
 * and reduced once per 256 values of k.  A small result is cut as for Evaluator_DotPlainDevice, the rule being asked with
 * size ceil(rows / 4) ceil(cols / 4) K N threads that each add `inner` terms: slices of the inner index are computed by separate
 * workgroups into pool scratch [slices][size][rows cols][K][N], which a second launch adds; the words do not depend on it.
 * Measured on one MI355X at size 2 (profiles/matmul_plain_items.txt): 2.35 - 2.45 times the mapped route at N = 65536, K = 15 from
 * 4 x 16 x 4 on, with either flag or both, and 1.49 - 1.92 times at N = 8192, K = 3 from 8 x 16 x 8 on; slower than it at rows =
 * cols = 1 (0.86 of it at N = 8192, 0.45 at N = 65536: use Evaluator_DotPlainDevice) and at N = 8192, 4 x 16 x 4 (0.57: the rule
 * cuts the 2 K N threads of the one tile into 4 slices and a second launch).  Sizes other than 2 and the rings below N = 128: not measured. */
SHL_FUNC Evaluator_MatMulPlainItems(void *thisptr, const uint64_t *device_plain, void *encrypted, uint64_t rows, uint64_t inner, uint64_t cols,
                                    uint64_t flags, double scale, void *destination);
/* Library extension: a matrix of SCALAR weights times a matrix of ciphertexts, out[i][j] = sum_k W[i][k] X[k][j] for i < rows,
 * j < cols, k < inner - the dense layer applied to many blocks at once, one ciphertext per (feature, block).  It is
 * Evaluator_MatMulPlainItems with one value in every slot of a plaintext, held as that value and not as [K][N] words, and
 * Evaluator_DotScalarsDevice with a column index.  encrypted, destination, flags bits 0 and 1 (with the transposed-use note) and
 * `scale` are Evaluator_MatMulPlainItems'.
 * flags bit 2 clear - WIDE weights: device_weights = [rows * inner][K] 64-bit words at the ciphertext's level, weight (i, k) at
 * i * inner + k: what CKKSEncoder_EncodeScalars / CKKSEncoder_EncodeIntegerScalars / Evaluator_LiftScalars write.  `scale` (CKKS) is
 * the scale the scalars were encoded at.
 * flags bit 2 set - NARROW weights: device_weights = [rows * inner] signed 32-bit integers; the weight is the constant polynomial
 * with that integer value, one 4-byte word for all K primes: it stands for the K words w mod q_k.  For CKKS these are the words
 * CKKSEncoder_EncodeIntegerScalars(w) gives - the words of scale 1.0 - whenever w >= -q_k, that is for every weight when no prime
 * of the level is below 2^31 (for a smaller prime and w < -q_k that producer follows the reference's Encode5, whose 64-bit sum
 * q_k + w wraps) - and `scale` is metadata only: the 2^s the caller quantised with, which becomes part of the result's scale
 * (ct.scale * scale, with the reference's bound check).  For BFV / BGV it stands for
 * Evaluator_LiftScalars(w mod t) for w inside the centred range of the lift, -(t - ceil(t / 2)) <= w < ceil(t / 2); outside it the
 * result is unspecified, as for any unvalidated device plaintext.
 * Any other bit is SHL_E_INVALIDARG.  Both forms must be 16-byte aligned, are not validated, and from N = 128 on are read through
 * the constant cache: they must have been WRITTEN BY SOMETHING EARLIER ON THE STREAM, as Evaluator_DotScalarsDevice's scalars.
 * Contract: output item (i, j) equals, word for word and in its metadata, Evaluator_MatMulPlainItems with the same bits 0 and 1 on
 * [rows * inner][K][N] plaintexts each filled with its weight's K words - hence the reference's multiply_plain_inplace per pair and
 * then add_many.  With cols = 1 and flags = 0 the words are Evaluator_DotScalarsDevice's.  The narrow form's words are the wide
 * form's on the words its weights stand for: the arithmetic is exact modulo each prime.
 * Metadata, the settle-before-read of an operand, Evaluator_SetTransparentCheck on the result batch and "a failed check leaves the
 * destination untouched" are Evaluator_MatMulPlainItems'.  SHL_E_POINTER for a NULL handle.  SHL_E_INVALIDARG: rows, inner or
 * cols == 0; rows * inner, inner * cols or rows * cols >= 2^32; the ciphertext's batch != inner * cols; the destination's batch !=
 * rows * cols; destination == encrypted; NULL or misaligned device_weights; device_weights overlapping the words of either
 * ciphertext; a coefficient-form ciphertext; an invalid or foreign ciphertext; a scale out of bounds; a result too large for one
 * launch.  The call is enqueued on the evaluator's stream without a host round trip and records under Evaluator_BeginCapture.
 * One thread holds a 16-byte coefficient pair of one plane, one prime and one output column for a tile of R consecutive output rows
 * - 4 for wide, 8 for narrow weights - and uses each loaded ciphertext pair for all of them.  Wide products are accumulated as plain 128-bit integers and reduced once
 * per 256 values of k.  A narrow weight is used as u = w + 2^31, unsigned: sum a u and sum a are accumulated exactly as 128-bit
 * integers - a product is two 32 x 32 multiplies where the wide form's compiles to six multiply instructions - and sum a w = sum a u - 2^31 sum a is reduced to
 * canonical words once per 1024 values of k.  A small result is cut as for Evaluator_DotPlainDevice, the rule being asked with
 * size ceil(rows / R) cols K N / 2 threads that each add `inner` terms; the words do not depend on it.
 * Measured on one MI355X at size 2 (profiles/matmul_scalars.txt), cols in {1, 4, 16}: at N = 65536, K = 15 the wide form is 1.7 - 6.6
 * times Evaluator_MatMulPlainItems' kernel on the expanded plaintexts and runs at 2.0 Tmac/s from 8 rows on, bound by its 64 x 64
 * multiplies; the narrow form is 1.27 - 1.30 times the wide form there (2.3 - 2.6 Tmac/s) and up to 1.58 times at N = 8192, K = 3.
 * At cols = 1 the wide form is not slower than Evaluator_DotScalarsDevice's kernel at any measured shape beyond the spread of the
 * samples.  The narrow form is slower than the wide one with a single row (0.67 - 0.99 at eight of nine shapes: seven of its eight
 * rows are dead) and at N = 8192, 8 x 16 x 1 and 8 x 16 x 4 (0.86 and 0.55: its fewer threads; at the second they are cut into
 * slices and a second launch).  Sizes other than 2 and the rings below N = 128: not measured. */
SHL_FUNC Evaluator_MatMulScalarsItems(void *thisptr, const void *device_weights, void *encrypted, uint64_t rows, uint64_t inner, uint64_t cols,
                                      uint64_t flags, double scale, void *destination);
/* Library extension: a 2-D convolution of SCALAR weights over a grid of ciphertexts, one ciphertext per (channel, pixel) with the
 * samples in the slots - the convolutional layer as one call and one pass, with no gathered (im2col) batch and with zero padding.
 * With OH = (height + 2 pad_h - kernel_h) / stride_h + 1, OW likewise and inner = in_channels * kernel_h * kernel_w:
 *   out(o, y', x') = sum_{c, dy, dx} W[o][(c * kernel_h + dy) * kernel_w + dx] * X(c, y' stride_h + dy - pad_h, x' stride_w + dx - pad_w)
 * over the taps that fall inside the image.  encrypted: a batch of in_channels * height * width items, item (c, y, x) at
 * (c * height + y) * width + x, of any size >= 2, at any level, in NTT form (CKKS, BGV, or BFV after Evaluator_TransformToNTT2).
 * destination: another handle of out_channels * OH * OW items, item (o, y', x') at (o * OH + y') * OW + x'.  `shape` is host memory.
 * flags bit 0: the input is stored channel-last, item (c, y, x) at (y * width + x) * in_channels + c; bit 1: the result is stored
 * channel-last, item (o, y', x') at (y' * OW + x') * out_channels + o; the layouts are strides of the one kernel, no data is moved.
 * Bit 2: NARROW weights, [out_channels * inner] signed 32-bit integers; otherwise WIDE, [out_channels * inner][K] 64-bit words.
 * Both forms, `scale`, their producers, their 16-byte alignment and "WRITTEN BY SOMETHING EARLIER ON THE STREAM" are exactly
 * Evaluator_MatMulScalarsItems'.  Any other bit is SHL_E_INVALIDARG.
 * Contract: output item (o, y', x') equals, word for word and in its metadata, Evaluator_DotPlainMapped over the map whose row for
 * that item names, for every tap inside the image, the input item and plaintext o * inner + (c * kernel_h + dy) * kernel_w + dx of
 * [out_channels * inner][K][N] plaintexts each filled with its weight's K words - hence the reference's multiply_plain_inplace per
 * tap and then add_many.  With a 1 x 1 kernel, stride 1 and no padding the words are Evaluator_MatMulScalarsItems' at rows =
 * out_channels, inner = in_channels, cols = height * width (flags as given); with kernel = the whole image, no padding and a
 * channel-first input they are its words at cols = 1.
 * Metadata, the settle-before-read of an operand, Evaluator_SetTransparentCheck on the result batch and "a failed check leaves the
 * destination untouched" are Evaluator_MatMulScalarsItems'.  SHL_E_POINTER for a NULL handle.  SHL_E_INVALIDARG: a NULL shape; an
 * extent or stride of 0; pad_h >= kernel_h or pad_w >= kernel_w (so every output has a tap inside the image and no transparent
 * item is made by construction); height + 2 pad_h < kernel_h, and likewise the width; one of C H W, OC OH OW, OC inner >= 2^32,
 * or inner OH OW >= 2^32 (the terms of one launch are numbered in 32 bits); the ciphertext's batch != C H W; the destination's
 * batch != OC OH OW; destination == encrypted; NULL or misaligned device_weights; device_weights overlapping the words of either
 * ciphertext; a coefficient-form ciphertext; an invalid or foreign ciphertext; a scale out of bounds; a result too large for one
 * launch.  Dilation and groups: not provided.  The call is enqueued on the evaluator's stream without a host round trip and
 * records under Evaluator_BeginCapture.
 * One thread holds a 16-byte coefficient pair of one plane, one prime and one output position for a tile of R consecutive output
 * channels - 4 for wide, 8 for narrow weights - with Evaluator_MatMulScalarsItems' sums and reductions, once per 256 / 1024 EXECUTED
 * taps.  The taps of an output position inside the image are a rectangle of the kernel, found once per thread; taps outside it are
 * neither read nor multiplied.  A small result is cut as for Evaluator_DotPlainDevice, the rule being asked with
 * size ceil(OC / R) OH OW K N / 2 threads that each add `inner` terms; a slice is a range of the term index (c * kernel_h + dy) *
 * kernel_w + dx, and the words do not depend on the cut.
 * Measured on one MI355X at size 2 (profiles/conv2d_scalars.txt) against the route without this call - the Evaluator_SumItemsMapped
 * gather into an im2col batch, then Evaluator_MatMulScalarsItems - on raw words: at N = 65536, K = 15, 3 x 3 over 8 channels of
 * 8 x 8 with 8 and 16 output channels and 5 x 5, stride 2, over one channel of 28 x 28 with 5, the wide form is 1.27 - 1.83 times and
 * the narrow form 1.31 - 1.84 times the two calls, in 12.6 - 23.7 GB of operands where the two calls hold 53.4 - 80.3 GB; at N = 8192,
 * K = 3, 1.34 - 2.04 times.  Slower than Evaluator_MatMulScalarsItems ALONE on an already gathered batch at N = 65536: the wide form
 * runs at 0.94 - 0.95 of its rate at the 3 x 3 shapes (2.25 - 2.30 against 2.40 - 2.42 Tmac/s), the narrow form at 0.84 - 0.86 (3.12
 * against 3.72) - the same bytes come from HBM, since the caches do not catch the re-reads of an item by neighbouring outputs, and
 * the walk from tap to tap costs 2.7 times the scalar instructions (wide) or 14 % more vector instructions and a wave (narrow).  The
 * operand loads carry no non-temporal hint: with it 1 % is gained at the 3 x 3 shapes at N = 65536 and 4 - 10 % lost at 28 x 28 and at
 * N = 8192.  Sizes other than 2 and the rings below N = 128: not measured. */
typedef struct
{
    uint64_t in_channels, height, width, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w;
} SHL_CONV2D;
SHL_FUNC Evaluator_Conv2dScalarsItems(void *thisptr, const void *device_weights, void *encrypted, const SHL_CONV2D *shape, uint64_t flags,
                                      double scale, void *destination);
SHL_FUNC Evaluator_Square(void *thisptr, void *encrypted, void *destination, void *pool);
SHL_FUNC Evaluator_Relinearize(void *thisptr, void *encrypted, void *relinKeys, void *destination, void *pool);
SHL_FUNC Evaluator_ModSwitchToNext1(void *thisptr, void *encrypted, void *destination, void *pool);
SHL_FUNC Evaluator_ModSwitchTo1(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *pool);
SHL_FUNC Evaluator_RescaleToNext(void *thisptr, void *encrypted, void *destination, void *pool);
SHL_FUNC Evaluator_RescaleTo(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *pool);
SHL_FUNC Evaluator_ModReduceToNext(void *thisptr, void *encrypted, void *destination, void *pool);
SHL_FUNC Evaluator_ModReduceTo(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *pool);
SHL_FUNC Evaluator_TransformToNTT2(void *thisptr, void *encrypted, void *destination_ntt);
SHL_FUNC Evaluator_TransformFromNTT(void *thisptr, void *encrypted_ntt, void *destination);
SHL_FUNC Evaluator_ApplyGalois(void *thisptr, void *encrypted, uint32_t galois_elt, void *galoisKeys, void *destination, void *pool);
SHL_FUNC Evaluator_RotateRows(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *destination, void *pool);
SHL_FUNC Evaluator_RotateColumns(void *thisptr, void *encrypted, void *galois_keys, void *destination, void *pool);
SHL_FUNC Evaluator_RotateVector(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *destination, void *pool);
SHL_FUNC Evaluator_ComplexConjugate(void *thisptr, void *encrypted, void *galoisKeys, void *destination, void *pool);
SHL_FUNC Evaluator_ContextUsingKeyswitching(void *thisptr, bool *using_keyswitching);

/* ------------------------------------------------------------------------------------------------
 * 1b. Digit-parallel key switching over the GPUs of one node (BASELINE configs[4]).
 * switch_key_inplace (native/src/seal/evaluator.cpp:2561-2867) is linear in the decomposition digits J up to its
 * mod-down tail, so the digits can be spread over ranks: every rank holds the same ciphertext, computes the
 * canonical partial sums S_k[I] = sum_{J in its range} NTT_I(t_J mod q_I) * key[J][k][I] for all K+1 target moduli
 * (`*Partial`), the ranks add their buffers (ONE all-reduce of 2 (K+1) N words per ciphertext, done by the caller,
 * e.g. torch.distributed.all_reduce over RCCL), and every rank finishes locally (`*Finish`: reduce mod q_I, mod-down by
 * the special prime, accumulate into (c0, c1)).  device_acc = caller-owned device buffer of Evaluator_SwitchKeyAccWords
 * 64-bit words; parts = number of summed buffers (<= 8: eight residues below 2^60 still fit one word).
 * Results equal Evaluator_Relinearize / Evaluator_ApplyGalois bit for bit.  CKKS at the two-pass sizes: `*Finish` may leave the
 * mod-down pending exactly as Evaluator_Relinearize does (deferred key-switch tail, below: a rescale on the same evaluator then
 * folds both divisions); the reduced sums are copied first, by a kernel QUEUED on the evaluator's stream: device_acc is read
 * asynchronously, so a caller that owns the buffer on another stream (a torch tensor, a communicator's receive buffer) must
 * not overwrite or free it before the evaluator's stream has passed this call - wait for an event recorded on that stream
 * after `*Finish`, or reuse the buffer only from work queued on the same stream (seal_amd/shard.py does the latter). */
SHL_FUNC Evaluator_SwitchKeyAccWords(void *thisptr, void *encrypted, uint64_t *words);
SHL_FUNC Evaluator_RelinearizePartial(void *thisptr, void *encrypted /* size 3 */, void *relinKeys, uint64_t digit_first,
                                      uint64_t digit_count, uint64_t *device_acc);
SHL_FUNC Evaluator_RelinearizeFinish(void *thisptr, void *encrypted, uint64_t *device_acc, uint64_t parts);
SHL_FUNC Evaluator_ApplyGaloisPartial(void *thisptr, void *encrypted /* size 2 */, uint32_t galois_elt, void *galoisKeys,
                                      uint64_t digit_first, uint64_t digit_count, uint64_t *device_acc);
SHL_FUNC Evaluator_ApplyGaloisFinish(void *thisptr, void *encrypted, uint64_t *device_acc, uint64_t parts);

/* ------------------------------------------------------------------------------------------------
 * 1c. The same with the exchange INSIDE the library: RCCL over xGMI, one process per GPU, collectives enqueued on the
 * evaluator's stream (no host synchronisation between the partial sums, the exchange and the mod-down).  The reference
 * has no counterpart (it is a single-host library); the loop being distributed is native/src/seal/evaluator.cpp:2663-2755
 * (digits) and 2806-2864 (target moduli).
 *   Comm_GetUniqueId     rank 0 draws the 128-byte RCCL id and hands it to the other ranks out of band
 *   Comm_Create          ncclCommInitRank on the calling thread's current device (collective over all ranks; nranks <= 8);
 *                        nranks == 1 also works without RCCL (loopback).  librccl.so.1 is loaded at run time.
 *   Comm_DigitRange      the contiguous share [first, first + count) of `digits` this rank multiplies
 *   Evaluator_BroadcastKeyDigits  one-time key distribution: `device_staging` (K*2*L*N words on every rank; on `root` the key
 *                        [digit][2][L][N]) is broadcast, every rank keeps its own digits resident
 *   Evaluator_*DigitParallel      relinearize / apply_galois / rotate_vector; every rank calls with equal ciphertexts.
 *     exchange 0: ONE all-reduce of 2 (K+1) N words per ciphertext, every rank runs the whole mod-down;
 *     exchange 1 (CKKS): reduce-scatter of the K data moduli's sums by owner + all-reduce of the special-prime component +
 *                 mod-down of the rank's own moduli + all-gather of the increments - the same bytes on the wire, the mod-down
 *                 divided by the number of ranks (BFV / BGV fall back to exchange 0).
 *   Results are bit-identical to Evaluator_Relinearize / Evaluator_ApplyGalois / Evaluator_RotateVector on one GPU.
 *   Evaluator_SwitchKeySlots / PackTargets / FinishOwned / AddGathered are the local phases of exchange 1 (layouts in
 *   seal_amd/csrc/evaluator.h); with them a caller can run the exchange through its own collective library. */
SHL_FUNC Comm_GetUniqueId(uint8_t *id128);
SHL_FUNC Comm_RcclAvailable(bool *available);
SHL_FUNC Comm_Create(const uint8_t *id128, int nranks, int rank, void **comm);
SHL_FUNC Comm_Destroy(void *comm);
SHL_FUNC Comm_Info(void *comm, int *nranks, int *rank, bool *loopback);
SHL_FUNC Comm_DigitRange(void *comm, uint64_t digits, uint64_t *first, uint64_t *count);
SHL_FUNC Comm_AllReduceWords(void *comm, uint64_t *device_words, uint64_t count, void *hip_stream);
SHL_FUNC Comm_BroadcastWords(void *comm, uint64_t *device_words, uint64_t count, int root, void *hip_stream);
SHL_FUNC Evaluator_RelinearizeDigitParallel(void *thisptr, void *encrypted, void *relinKeys, void *comm, int exchange, void *destination);
SHL_FUNC Evaluator_ApplyGaloisDigitParallel(void *thisptr, void *encrypted, uint32_t galois_elt, void *galoisKeys, void *comm, int exchange,
                                            void *destination);
SHL_FUNC Evaluator_RotateVectorDigitParallel(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *comm, int exchange,
                                             void *destination);
SHL_FUNC Evaluator_BroadcastKeyDigits(void *thisptr, void *kswitch_keys, uint64_t index, uint64_t *device_staging, void *comm, int root);
SHL_FUNC Evaluator_SwitchKeySlots(void *thisptr, void *encrypted, uint64_t nranks, uint64_t *slots);
SHL_FUNC Evaluator_SwitchKeyPackTargets(void *thisptr, void *encrypted, const uint64_t *device_acc, uint64_t nranks, uint64_t *device_send,
                                        uint64_t *device_special);
SHL_FUNC Evaluator_SwitchKeyFinishOwned(void *thisptr, void *encrypted, const uint64_t *device_recv, const uint64_t *device_special,
                                        uint64_t nranks, uint64_t rank, uint64_t *device_own);
SHL_FUNC Evaluator_SwitchKeyAddGathered(void *thisptr, void *encrypted, const uint64_t *device_all, uint64_t nranks);

/* ------------------------------------------------------------------------------------------------
 * 2. Per-kernel seam on raw device slabs (device pointers; `stream` is a hipStream_t or NULL)
 * ---------------------------------------------------------------------------------------------- */

/* ntt_negacyclic_harvey[_lazy] / inverse_ntt_negacyclic_harvey[_lazy] (util/ntt.cpp:394-475) over
 * `polys` polynomials of `comps` consecutive RNS components starting at pool prime `first_prime`;
 * data = [polys][comps][N].  lazy != 0 leaves the reference's lazy range ([0,4q) fwd / [0,2q) inv). */
SHL_FUNC shl_ntt_forward(void *context, uint64_t *data, uint64_t polys, uint64_t comps, uint64_t first_prime, int lazy, void *stream);
SHL_FUNC shl_ntt_inverse(void *context, uint64_t *data, uint64_t polys, uint64_t comps, uint64_t first_prime, int lazy, void *stream);
/* dyadic_product_coeffmod (util/polyarithsmallmod.cpp:226-284): r = a .* b, operands may be lazy (< 4q) */
SHL_FUNC shl_dyadic_product(void *context, const uint64_t *a, const uint64_t *b, uint64_t *r, uint64_t polys, uint64_t comps, uint64_t first_prime, void *stream);
/* The kernels of Evaluator_SumItems (plain == NULL) / Evaluator_DotPlainDevice on raw words at one level: a = [size][batch][K][N],
 * plain = [batch][K][N], r = [size][batch / group][K][N], r distinct from the operands.  slices: 0 = the library's rule, 1 = one
 * launch, 2 .. min(group, 64) = that cut of the group, with scratch of slices * size * (batch / group) * K * N words.  slices_used
 * (may be NULL) receives the slices run; r == NULL only answers that.  Nothing is validated beyond the shape. */
SHL_FUNC shl_reduce_items(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *plain, uint64_t *r, uint64_t size,
                          uint64_t batch, uint64_t group, uint64_t slices, uint64_t *scratch, uint64_t *slices_used, void *stream);
/* terms the lazy accumulators of those kernels take between two reductions (sums: 16; products: 256) */
SHL_FUNC shl_reduce_flush_intervals(uint64_t *sum_terms, uint64_t *dot_terms);
/* The kernels of Evaluator_DotItems on raw words at one level: x, y = [2][batch][K][N], r = [3][batch / group][K][N], r distinct
 * from the operands; y == x selects the square kernel (x is read once).  slices, scratch (slices * 3 * (batch / group) * K * N
 * words), slices_used and r == NULL: as shl_reduce_items.  Nothing is validated beyond the shape. */
SHL_FUNC shl_dot_items(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t batch,
                       uint64_t group, uint64_t slices, uint64_t *scratch, uint64_t *slices_used, void *stream);
/* items the lazy accumulators of that kernel take between two reductions (128: the middle polynomial adds two products per item) */
SHL_FUNC shl_dot_items_flush_interval(uint64_t *items);
/* The kernels of the *Mapped reductions on raw words at one level.  kind 0: the sum, a = [size][a_batch][K][N], b unused; kind 1:
 * the plaintext dot product, a as before, b = [b_batch][K][N]; kind 2: the ciphertext dot product, a = [2][a_batch][K][N],
 * b = [2][b_batch][K][N], size ignored (the result has 3 planes; b == a with a one-list map selects the square kernel).
 * r = [size or 3][rows][K][N], distinct from the operands.  a_batch / b_batch must be the map's first_batch / second_batch.  slices:
 * 0 = the library's rule (above), 1 = one launch, 2 .. min(longest_row, 64) = that cut of the longest row, with scratch of
 * slices * (size or 3) * rows * K * N words; the slices run are ceil(longest_row / ceil(longest_row / slices)).  slices_used (may be
 * NULL) receives them; r == NULL only answers that.  Nothing is validated beyond the shape. */
SHL_FUNC shl_reduce_mapped(void *context, uint64_t chain_index, int kind, const uint64_t *a, uint64_t a_batch, const uint64_t *b,
                           uint64_t b_batch, uint64_t *r, uint64_t size, void *item_map, uint64_t slices, uint64_t *scratch,
                           uint64_t *slices_used, void *stream);
/* The kernel of Evaluator_DotScalarsMapped on raw words at one level, with shl_reduce_mapped's conventions: weights =
 * [weight_count][K] 64-bit words or, narrow != 0, [weight_count] signed 32-bit integers; a = [size][a_batch][K][N]; r =
 * [size][rows][K][N], distinct from the operands.  a_batch / weight_count must be the map's first_batch / second_batch.  slices: 0 =
 * the library's rule (size * rows * K * N / 2 threads), 1 = one launch, 2 .. min(longest_row, 64) = that cut of the longest row, with
 * scratch of slices * size * rows * K * N words; slices_used (may be NULL) receives the slices run; r == NULL only answers that.
 * Nothing is validated beyond the shape.  shl_dot_scalars_mapped_info: the terms between two reductions (wide 256, narrow 1024). */
SHL_FUNC shl_dot_scalars_mapped(void *context, uint64_t chain_index, const void *weights, uint64_t weight_count, int narrow, const uint64_t *a,
                                uint64_t a_batch, uint64_t *r, uint64_t size, void *item_map, uint64_t slices, uint64_t *scratch,
                                uint64_t *slices_used, void *stream);
SHL_FUNC shl_dot_scalars_mapped_info(uint64_t *flush, uint64_t *narrow_flush);
/* The kernel of Evaluator_DotScalarsDevice on raw words at one level: a = [size][batch][K][N], scalars = [rows][batch][K],
 * r = [size][rows][K][N], distinct from the operands.  slices: 0 = the library's rule, 1 = one launch, 2 .. min(batch, 64) = that cut
 * of the batch; the scratch comes from the pool.  slices_used (may be NULL) receives the slices run; r == NULL only answers that.
 * Nothing is validated beyond the shape.  shl_dot_scalars runs on the NULL stream and returns when the work is done;
 * shl_dot_scalars_tile enqueues on `stream` with a row tile of 2, 4 or 8 output rows per thread (0: the library's) - the sweep of
 * tools/dot_scalars_rate.py.  shl_dot_scalars_info: the library's row tile and the items between two reductions (256). */
SHL_FUNC shl_dot_scalars(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *scalars, uint64_t *r, uint64_t size,
                         uint64_t rows, uint64_t batch, uint64_t slices, uint64_t *slices_used);
SHL_FUNC shl_dot_scalars_tile(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *scalars, uint64_t *r, uint64_t size,
                              uint64_t rows, uint64_t batch, uint64_t slices, uint64_t *slices_used, uint64_t row_tile, void *stream);
SHL_FUNC shl_dot_scalars_info(uint64_t *row_tile, uint64_t *flush);
/* The kernel of Evaluator_MatMulItems on raw words at one level: x = [2][rows * inner][K][N], y = [2][inner * cols][K][N] (items
 * [cols][inner] when y_transposed != 0), r = [3][rows * cols][K][N], distinct from the operands; x == y is allowed.  slices: 0 = the
 * library's rule, 1 = one launch, 2 .. min(inner, 64) = that cut of the inner index; the scratch comes from the pool.  slices_used
 * (may be NULL) receives the slices run; r == NULL only answers that.  Nothing is validated beyond the shape.  shl_matmul_items runs
 * on the NULL stream and returns when the work is done; shl_matmul_items_tile enqueues on `stream` with the tile
 * tile_rows << 8 | tile_cols of output rows x columns per thread - 1 x 1 and 2 x 2 (a thread holds a 16-byte coefficient pair) and
 * 2 x 4 (one coefficient) are built, 0 is the library's - to which
 * 1 << 16 / 2 << 16 may be added for operand loads with / without the non-temporal hint (neither: the library's choice) - the sweep
 * of tools/matmul_items_rate.py.  shl_matmul_items_info: the library's tile and the values of k between two reductions (128). */
SHL_FUNC shl_matmul_items(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t rows, uint64_t inner,
                          uint64_t cols, int y_transposed, uint64_t slices, uint64_t *slices_used);
SHL_FUNC shl_matmul_items_tile(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t rows,
                               uint64_t inner, uint64_t cols, int y_transposed, uint64_t slices, uint64_t *slices_used, uint64_t tile,
                               void *stream);
SHL_FUNC shl_matmul_items_info(uint64_t *tile_rows, uint64_t *tile_cols, uint64_t *flush);
/* The kernel of Evaluator_MatMulPlainItems on raw words at one level: pl = [rows * inner][K][N], a = [size][inner * cols][K][N]
 * (items [cols][inner] with flags bit 0), r = [size][rows * cols][K][N] (items [cols][rows] with flags bit 1), distinct from the
 * operands; 1 <= size <= 16, any other bit of flags is refused.  slices: 0 = the library's rule, 1 = one launch, 2 .. min(inner, 64)
 * = that cut of the inner index; the scratch comes from the pool.  slices_used (may be NULL) receives the slices run; r == NULL only
 * answers that.  Nothing is validated beyond the shape.  shl_matmul_plain_items runs on the NULL stream and returns when the work
 * is done; shl_matmul_plain_items_tile enqueues on `stream` with the tile tile_rows << 8 | tile_cols of output rows x columns per
 * thread - 1 x 1 (a thread holds a 16-byte coefficient pair) and 2 x 4, 4 x 4, 4 x 8 (one coefficient) are built, 0 is the
 * library's, anything else is SHL_E_INVALIDARG - to which 1 << 16 / 2 << 16 may be added for operand loads with / without the
 * non-temporal hint (neither: the library's choice) - the sweep of tools/matmul_plain_items_rate.py.
 * shl_matmul_plain_items_info: the library's tile and the values of k between two reductions (256). */
SHL_FUNC shl_matmul_plain_items(void *context, uint64_t chain_index, const uint64_t *pl, const uint64_t *a, uint64_t *r, uint64_t size,
                                uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used);
SHL_FUNC shl_matmul_plain_items_tile(void *context, uint64_t chain_index, const uint64_t *pl, const uint64_t *a, uint64_t *r, uint64_t size,
                                     uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used,
                                     uint64_t tile, void *stream);
SHL_FUNC shl_matmul_plain_items_info(uint64_t *tile_rows, uint64_t *tile_cols, uint64_t *flush);
/* The kernel of Evaluator_MatMulScalarsItems on raw words at one level: weights = [rows * inner][K] 64-bit words or, with flags bit
 * 2, [rows * inner] signed 32-bit integers; a, r, size, flags bits 0 and 1, slices and slices_used as for shl_matmul_plain_items.
 * slices_used receives the slices run: of a forced cut those that ceil(inner / slices) values of k each leave non-empty.
 * Nothing is validated beyond the shape.  shl_matmul_scalars runs on the NULL stream and returns when the work is done;
 * shl_matmul_scalars_tile enqueues on `stream` with row_tile output rows per thread - 4 and 8 are built, 0 is the library's for the
 * form, anything else is SHL_E_INVALIDARG - the sweep of tools/matmul_scalars_rate.py.
 * shl_matmul_scalars_info: the library's row tile for wide and for narrow weights and the values of k between two reductions of
 * each form (256 and 1024). */
SHL_FUNC shl_matmul_scalars(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                            uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used);
SHL_FUNC shl_matmul_scalars_tile(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                 uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used,
                                 uint64_t row_tile, void *stream);
SHL_FUNC shl_matmul_scalars_info(uint64_t *row_tile, uint64_t *narrow_row_tile, uint64_t *flush, uint64_t *narrow_flush);
/* The kernel of Evaluator_Conv2dScalarsItems on raw words at one level: weights = [OC * inner][K] 64-bit words or, with flags bit 2,
 * [OC * inner] signed 32-bit integers, inner = C * kernel_h * kernel_w; a = [size][C * H * W][K][N] (channel-last items with flags
 * bit 0), r = [size][OC * OH * OW][K][N] (channel-last items with bit 1); shape is host memory.  slices == 0: the library's rule;
 * otherwise 1 <= slices <= min(inner, 64) ranges of the term index, anything else is SHL_E_INVALIDARG; slices_used receives the
 * slices run: of a forced cut those that ceil(inner / slices) terms each leave non-empty.  r == NULL: the query.  Nothing is
 * validated beyond the shape.  shl_conv2d_scalars runs on the NULL stream and returns when the work is done;
 * shl_conv2d_scalars_tile enqueues on `stream` with row_tile output channels per thread (0, 4, 8 as shl_matmul_scalars_tile) and
 * operand loads with (hint 1) or without (hint 2) the non-temporal hint, 0 = the library's choice - the sweep of
 * tools/conv2d_scalars_rate.py.  The row tiles and flush intervals are those shl_matmul_scalars_info reports. */
SHL_FUNC shl_conv2d_scalars(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                            const SHL_CONV2D *shape, uint64_t flags, uint64_t slices, uint64_t *slices_used);
SHL_FUNC shl_conv2d_scalars_tile(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                 const SHL_CONV2D *shape, uint64_t flags, uint64_t slices, uint64_t *slices_used, uint64_t row_tile,
                                 uint64_t hint, void *stream);
/* GaloisTool::apply_galois (ntt_form == 0, util/galois.cpp:148) / apply_galois_ntt (!= 0, galois.cpp:192) */
SHL_FUNC shl_apply_galois(void *context, uint64_t chain_index, int ntt_form, uint32_t galois_elt, const uint64_t *in, uint64_t *out, uint64_t polys, void *stream);
/* RNSTool stages (util/rns.cpp) on one level, `polys` polynomials each [comps][N]:
 *   0 fastbconv_m_tilde  q -> Bsk U {m~}      (rns.cpp:1086)     in K comps,        out |Bsk|+1
 *   1 sm_mrq             Bsk U {m~} -> Bsk    (rns.cpp:979)      in |Bsk|+1,        out |Bsk|
 *   2 fast_floor         q U Bsk -> Bsk       (rns.cpp:1041)     in K+|Bsk|,        out |Bsk|
 *   3 fastbconv_sk       Bsk -> q             (rns.cpp:903)      in |Bsk|,          out K
 *   4 divide_and_round_q_last_inplace         (rns.cpp:789)      in K,              out K-1
 *   5 divide_and_round_q_last_ntt_inplace     (rns.cpp:830)      in K,              out K-1
 *   6 lift       = stages 0 then 1 as the one fused kernel Evaluator::multiply runs          in K,        out |Bsk|
 *   7 floor_sk   = (x t), then stages 2 then 3 as the one fused kernel (evaluator.cpp:549-566)
 *                                                                 in K+|Bsk| (the q part first, as stage 2), out K
 * Stages 0-3, 6 and 7 exist for BFV contexts only. */
SHL_FUNC shl_rns_stage(void *context, uint64_t chain_index, int which, const uint64_t *in, uint64_t *out, uint64_t polys, void *stream);
/* ------------------------------------------------------------------------------------------------
 * 1d. The container surface a sealc binding uses besides the hot path (seal_amd/csrc/capi_containers.cpp)
 * ----------------------------------------------------------------------------------------------
 * Same names and argument lists as native/src/seal/c/{ciphertext,kswitchkeys,sealcontext,contextdata,encryptionparameters,
 * secretkey,publickey}.h unless a line says otherwise.  A word index addresses the device slab [poly][batch][K][N] (batch of one:
 * Ciphertext::data()); every call drains the device first (these are not hot-path functions).
 *
 * DELIBERATELY ABSENT from those seven headers (tests/test_cabi.py keeps both lists honest against the reference's headers: a sealc
 * function of these seven is declared in this file with the same argument types, or named in one of the two lists):
 *   Ciphertext_Pool, KSwitchKeys_Pool, SecretKey_Pool, PublicKey_Pool
 *                                     a MemoryPoolHandle has no device meaning (note (2) at the top)
 *   Ciphertext_Create1, SecretKey_Create1, PublicKey_Create1
 *                                     a device object is bound to a SEALContext when it is made: Ciphertext_Create3 /
 *                                     SecretKey_Create / PublicKey_Create take the context
 *   SecretKey_Data, PublicKey_Data    sealc returns a pointer to the member Plaintext / Ciphertext; the words are read with
 *                                     SecretKey_Get / PublicKey_Get and written with SecretKey_Set / PublicKey_Set
 *   EncParams_SetPlainModulus1        takes a Modulus handle; a Modulus travels as its 64-bit value here (EncParams_SetPlainModulus2)
 * SAME NAME, DIFFERENT ARGUMENTS (each for the reason given where it is declared):
 *   EncParams_GetCoeffModulus, EncParams_SetCoeffModulus, EncParams_GetPlainModulus     uint64_t values instead of Modulus handles
 *   SecretKey_Set, PublicKey_Set      take host words (section 1a); sealc's object-to-object assignment is SecretKey_Assign /
 *                                     PublicKey_Assign
 * Everything else of those headers is here or in sections 1 / 1a / 1b. */
/* Ciphertext (c/ciphertext.h:20-60).  Create4 / Create5: an empty ciphertext of batch 1 with parms_id set and room for 2 / `capacity`
 * polynomials (ciphertext.h:128-149).  SetParmsId takes the ids of the context's chain or parms_id_zero (E_INVALIDARG otherwise: a
 * device object names its level by pointer).  Resize4 is the .NET loader's resize(size, N, K): the geometry must be a level's. */
SHL_FUNC Ciphertext_Create4(void *context, uint64_t *parms_id, void *pool, void **cipher);
SHL_FUNC Ciphertext_Create5(void *context, uint64_t *parms_id, uint64_t capacity, void *pool, void **cipher);
SHL_FUNC Ciphertext_Reserve1(void *thisptr, void *context, uint64_t *parms_id, uint64_t size_capacity);
SHL_FUNC Ciphertext_Reserve2(void *thisptr, void *context, uint64_t size_capacity);
SHL_FUNC Ciphertext_Reserve3(void *thisptr, uint64_t size_capacity);
SHL_FUNC Ciphertext_SizeCapacity(void *thisptr, uint64_t *size_capacity);
SHL_FUNC Ciphertext_SetParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC Ciphertext_Resize2(void *thisptr, void *context, uint64_t size);
SHL_FUNC Ciphertext_Resize3(void *thisptr, uint64_t size);
SHL_FUNC Ciphertext_Resize4(void *thisptr, uint64_t size, uint64_t polyModulusDegree, uint64_t coeffModCount);
SHL_FUNC Ciphertext_GetDataAt1(void *thisptr, uint64_t index, uint64_t *data);
SHL_FUNC Ciphertext_GetDataAt2(void *thisptr, uint64_t poly_index, uint64_t coeff_index, uint64_t *data); /* batch item 0 */
SHL_FUNC Ciphertext_SetDataAt(void *thisptr, uint64_t index, uint64_t value);
SHL_FUNC Ciphertext_Release(void *thisptr);
/* KSwitchKeys (c/kswitchkeys.h:20-33).  GetKeyList: sealc hands out pointers into the object; here every digit of key `index` is
 * given out as a NEW PublicKey (the device key is one slab in the kernels' order) which the caller destroys with PublicKey_Destroy;
 * key_list == NULL returns the count only.  AddKeyList appends a key made of `count` PublicKey handles (0: an empty slot). */
SHL_FUNC KSwitchKeys_Create2(void *copy, void **kswitch_keys);
SHL_FUNC KSwitchKeys_Set(void *thisptr, void *assign);
SHL_FUNC KSwitchKeys_RawSize(void *thisptr, uint64_t *key_count);
SHL_FUNC KSwitchKeys_GetKeyList(void *thisptr, uint64_t index, uint64_t *count, void **key_list);
SHL_FUNC KSwitchKeys_ClearDataAndReserve(void *thisptr, uint64_t size);
SHL_FUNC KSwitchKeys_AddKeyList(void *thisptr, uint64_t count, void **key_list);
SHL_FUNC KSwitchKeys_GetParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC KSwitchKeys_SetParmsId(void *thisptr, uint64_t *parms_id);
/* SEALContext (c/sealcontext.h:28-40).  SEALContext_Create refuses what the reference would construct with parameters_set() ==
 * false (E_INVALIDARG, including parameters that are insecure for a sec_level of 128 / 192 / 256): an existing handle is a valid
 * context, ParametersSet is true and the error name / message are "success" / "valid".  A ContextData handle names one level of
 * the chain; it is owned by the library and valid as long as its context (ContextData_Destroy is accepted and does nothing, as
 * the pointers sealc returns belong to the SEALContext); NULL where the reference returns a null pointer. */
SHL_FUNC SEALContext_ParametersSet(void *thisptr, bool *params_set);
SHL_FUNC SEALContext_ParameterErrorName(void *thisptr, char *outstr, uint64_t *length);
SHL_FUNC SEALContext_ParameterErrorMessage(void *thisptr, char *outstr, uint64_t *length);
SHL_FUNC SEALContext_KeyContextData(void *thisptr, void **context_data);
SHL_FUNC SEALContext_FirstContextData(void *thisptr, void **context_data);
SHL_FUNC SEALContext_LastContextData(void *thisptr, void **context_data);
SHL_FUNC SEALContext_GetContextData(void *thisptr, uint64_t *parms_id, void **context_data);
/* ContextData (c/contextdata.h): array getters follow sealc's convention - *count carries the capacity in and the length out, a
 * NULL array returns the length only, a length of 0 means "not computed for these parameters" (CKKS has no coeff_div_plain_modulus,
 * BFV / BGV no upper_half_threshold).  ContextData_Parms returns a new EncryptionParameters (EncParams_Destroy), ContextData_Qualifiers
 * a new EncryptionParameterQualifiers (EPQ_Destroy; c/encryptionparameterqualifiers.h). */
SHL_FUNC ContextData_Destroy(void *thisptr);
SHL_FUNC ContextData_TotalCoeffModulus(void *thisptr, uint64_t *count, uint64_t *total_coeff_modulus);
SHL_FUNC ContextData_TotalCoeffModulusBitCount(void *thisptr, int *bit_count);
SHL_FUNC ContextData_Parms(void *thisptr, void **parms);
SHL_FUNC ContextData_Qualifiers(void *thisptr, void **epq);
SHL_FUNC ContextData_CoeffDivPlainModulus(void *thisptr, uint64_t *count, uint64_t *coeff_div);
SHL_FUNC ContextData_PlainUpperHalfThreshold(void *thisptr, uint64_t *puht);
SHL_FUNC ContextData_PlainUpperHalfIncrement(void *thisptr, uint64_t *count, uint64_t *puhi);
SHL_FUNC ContextData_UpperHalfThreshold(void *thisptr, uint64_t *count, uint64_t *uht);
SHL_FUNC ContextData_UpperHalfIncrement(void *thisptr, uint64_t *count, uint64_t *uhi);
SHL_FUNC ContextData_PrevContextData(void *thisptr, void **prev_data);
SHL_FUNC ContextData_NextContextData(void *thisptr, void **next_data);
SHL_FUNC ContextData_ChainIndex(void *thisptr, uint64_t *index);
SHL_FUNC ContextData_ParmsId(void *thisptr, uint64_t *parms_id); /* library extension: the level's parms_id without the temporary */
SHL_FUNC EPQ_Destroy(void *thisptr);
SHL_FUNC EPQ_ParametersSet(void *thisptr, bool *parameters_set);
SHL_FUNC EPQ_UsingFFT(void *thisptr, bool *using_fft);
SHL_FUNC EPQ_UsingNTT(void *thisptr, bool *using_ntt);
SHL_FUNC EPQ_UsingBatching(void *thisptr, bool *using_batching);
SHL_FUNC EPQ_UsingFastPlainLift(void *thisptr, bool *using_fast_plain_lift);
SHL_FUNC EPQ_UsingDescendingModulusChain(void *thisptr, bool *using_descending_modulus_chain);
SHL_FUNC EPQ_SecLevel(void *thisptr, int *sec_level);
/* EncryptionParameters (c/encryptionparameters.h:20-49): copy, assignment, parms_id (BLAKE2b-256, encryptionparams.cpp:117-147),
 * equality, and the wire format of EncryptionParameters::save / load (encryptionparams.cpp:15-122; all three compression modes) */
SHL_FUNC EncParams_Create2(void *copy, void **enc_params);
SHL_FUNC EncParams_Set(void *thisptr, void *assign);
SHL_FUNC EncParams_GetParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC EncParams_GetPlainModulus(void *thisptr, uint64_t *plain_modulus); /* (uint64_t, not a Modulus handle) */
SHL_FUNC EncParams_Equals(void *thisptr, void *otherptr, bool *result);
SHL_FUNC EncParams_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC EncParams_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
SHL_FUNC EncParams_Load(void *thisptr, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
/* SecretKey / PublicKey (c/secretkey.h, c/publickey.h): copies, parms_id, and SecretKey::save / PublicKey::save - the stream of the
 * key's Plaintext (L*N coefficients at the key level) resp. Ciphertext (size 2, key level, NTT form), byte for byte the reference's */
SHL_FUNC SecretKey_Create2(void *copy, void **secret_key);
SHL_FUNC SecretKey_Assign(void *thisptr, void *assign);
SHL_FUNC SecretKey_ParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC SecretKey_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC SecretKey_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
SHL_FUNC PublicKey_Create2(void *copy, void **public_key);
SHL_FUNC PublicKey_Assign(void *thisptr, void *assign);
SHL_FUNC PublicKey_ParmsId(void *thisptr, uint64_t *parms_id);
SHL_FUNC PublicKey_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
SHL_FUNC PublicKey_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
/* the pool of cached HBM blocks (the role of MemoryManager / MemoryPool, native/src/seal/memorymanager.h:75-265): give the
 * cached blocks back to the driver; counters for tests */
SHL_FUNC SealHip_ReleasePool(void);
/* Ciphertext_CopyFromHost / CopyToHost / CopyWordsToHost through pinned bounce buffers owned by the library instead of a
 * direct hipMemcpy on the caller's buffer, so that the caller's pages are never registered with the driver.  For hosts that
 * change the protection of their own buffers (integration/seal_evaluator_hip.cpp); process-wide, off by default. */
SHL_FUNC SealHip_SetStagedHostCopies(bool enabled);
SHL_FUNC SealHip_PoolStats(uint64_t *bytes_held, uint64_t *cross_stream_waits);
/* Diagnostics (opt-in: process-wide handlers belong to the host program, loading the library installs none).
 * SealHip_InstallAbortTrace(path) - or SEALHIP_ABORT_TRACE=<path> in the environment when the library is loaded -
 *   * installs a std::terminate handler: an exception that escapes where none may (a destructor, a host worker thread) prints its
 *     message before the handler that was installed before it runs (no HIP call is made: the runtime may be gone by then);
 *   * catches SIGABRT, appends the call stack of the aborting thread to `path` (the ROCm runtime aborts the process itself when the
 *     device reports a memory fault: its handler on the stack tells that case from a C++ one) and then lets the abort proceed
 *     with the default disposition.  A later call only changes the path. */
SHL_FUNC SealHip_InstallAbortTrace(const char *path);
/* Environment.  The product library reads twelve variables, each exercised by a test.  What tests and tools set beyond
 * them (thresholds, traces, chunk sizes of the emulated runs) only exists in development builds made with
 * -DSEALHIP_AB_SWITCHES (seal_amd/csrc/modarith.h: shl_ab_getenv); the A/B switches of settled measurements (superseded
 * kernels, fork / no-fork of the side streams, ...) are retired: DESIGN section 9.
 *   SEALHIP_NO_FP=1                  every prime on the 64-bit integer back end (no exact double-precision arithmetic for
 *                                    primes below 2^50); same words, slower.  Read when a SEALContext is created.
 *   SEALHIP_KS_EAGER_TAIL=1          key switches complete their mod-down before they return (no deferred tails, below)
 *   SEALHIP_KS_SPLIT=<parts>         cut the digits of a key switch into <parts> in-launch groups (small batches; default:
 *                                    chosen from the batch size)
 *   SEALHIP_NTT_FCHUNKS=<n>          workgroups per component of the single-launch transforms (N = 2^13, 2^14): tests force
 *                                    the per-workgroup loop at small batches with it
 *   SEALHIP_ENCRYPT_HOST_SAMPLING=1  encryption noise is sampled on the host with the reference's own sampler instead of the
 *                                    device kernels (same distribution and, for a seeded generator, the same words)
 *   SEALHIP_ABORT_TRACE=<file>       SealHip_InstallAbortTrace(<file>) when the library is loaded (Diagnostics, above)
 *   SEALHIP_KS_CHUNK=<items>         chunk size of a key switch over a large batch (below; 0 = never cut; default: the items
 *                                    that make 8192 pass-2 workgroups - 32 at N = 2^16 with 16 moduli)
 *   SEALHIP_KS_LANES=<1..4>          streams the chunks are dealt to (default 3; 1 = one after the other on the evaluator's stream)
 *   SEALHIP_KS_SCRATCH_CAP_MIB=<n>   upper bound of the key switch's intermediate (default 16384); chunk / lanes shrink to fit
 *   SEALHIP_LAZY_PRODUCT=0           tensor products are formed when Evaluator_Multiply is called (no deferred products, below)
 *   SEALHIP_LAZY_PRODUCT_MIN_WGS=<n> a product is deferred when its key switch would launch more than <n> second-pass workgroups
 *                                    (default 1024: the batches whose key switch runs as one digit group); tests reach the
 *                                    deferred form at small batches with 0, together with SEALHIP_KS_SPLIT=1
 *   SEALHIP_TAIL_P1_ORDER=0 / 1      first pass of the rounding tails (rescale, the key switch's mod-down, the two folded into one)
 *                                    at 2^13 <= N <= 2^16: 0 = one workgroup per target component, 1 = one workgroup per source
 *                                    tile with the target components in a loop (default: 1 for batches whose tiles fill the chip,
 *                                    0 below).  Same words either way; read once. */
/* Chunked key switching (round 5).  switch_key_inplace needs K (K + 1) half-transformed digits per ciphertext between its two
 * kernels (126 MB at N = 2^16, K = 15).  For a batch of 1.5 chunks or more (2^13 <= N <= 2^16, register-order keys, one digit group) the batch is cut
 * into chunks dealt round-robin to `lanes` streams forked from and joined to the evaluator's stream: the intermediate held
 * is lanes x chunk items whatever the batch (the reference holds O(K N) per ciphertext, evaluator.cpp:2561-2867); the lanes
 * hide the launch tails of the chunks (the step is as fast as with one launch over the batch, within +-1 %).  Same words as the
 * unchunked form.  While a graph is recorded the chunks stay on the recording stream.
 * Counters for tests and bench.py: calls that ran in chunks, chunks issued, the largest intermediate (bytes) any fused key switch
 * held since the previous query (the query resets it). */
SHL_FUNC SealHip_KsChunkStats(uint64_t *calls, uint64_t *chunks, uint64_t *scratch_bytes_max);
/* Deferred key-switch tails.  For CKKS and BFV at 2^13 <= N <= 2^16, Evaluator_Relinearize / ApplyGalois / RotateVector / RotateRows /
 * RotateColumns / ComplexConjugate (and, CKKS, the digit-parallel Evaluator_RelinearizeFinish / ApplyGaloisFinish and the *DigitParallel
 * forms with the all-reduce exchange) return with the mod-down by the special prime (evaluator.cpp:2806-2864) not yet run: the ciphertext
 * object keeps the key-switch sums next to its two polynomials.  Whatever needs the words next completes it first -
 * every Evaluator_* call on the object, Ciphertext_CopyToHost / Save / copies, Decryptor_Decrypt, destroying the evaluator,
 * Evaluator_SetStream, Evaluator_BeginCapture (tails from before the recording) and Evaluator_EndCapture (tails deferred inside
 * it and not consumed there become the recording's last work) - except Evaluator_RescaleToNext (in place) on the same evaluator, which performs the mod-down and
 * its own division by q_last with ONE transform per component instead of two (rns.cpp:830-901 folded in by linearity of the
 * transform; same words as the two separate steps) - and, for BFV, Evaluator_ModSwitchToNext1 (in place) on the same evaluator,
 * which does the mod-down and its own division (rns.cpp:789-828) in one element-wise pass over the inverse-transformed sums.  Metadata (size, parms_id, scale) is up to date at all times.  A deferred
 * tail runs on the stream of the evaluator that created it; a caller on another stream is made to wait for it.  Not thread
 * safe per object, like every other Ciphertext operation.  SEALHIP_KS_EAGER_TAIL=1 in the environment turns deferral off.
 * Counters for tests: tails folded into a rescale / completed on their own / discarded because the object was overwritten. */
SHL_FUNC SealHip_TailStats(uint64_t *folded, uint64_t *plain, uint64_t *dropped);
/* Deferred tensor products (round 6).  Evaluator_Multiply of two size-2 CKKS ciphertexts - into a THIRD object or in place (destination =
 * encrypted1, Evaluator_Square included) -, at the two-pass sizes and batches large enough for the un-split key switch, does not form the
 * product at once: the destination has its shape and metadata (size 3, scale, parms_id), its words are pending.  In the in-place forms
 * the destination's previous slab - its two polynomials - stays with the pending record and the destination gets a fresh slab; nothing is
 * copied.  Evaluator_Relinearize on the same evaluator then never stores the product - the third polynomial is formed inside the inverse
 * transform that opens the key switch, the first two inside the key switch's last epilogue (evaluator.cpp:604-663 folded into
 * 2561-2867; one kernel and the product's round trip through HBM less).  Anything else that touches the destination's words forms the
 * product first, and anything that writes, re-shapes or destroys a live OPERAND while a product of it is pending forms that product
 * first: the words are the reference's either way, at every point the caller can observe.  SEALHIP_LAZY_PRODUCT=0 in the environment
 * turns the deferral off.  Counters for tests: products consumed by a fused relinearisation / formed on their own / discarded because
 * the destination was overwritten. */
SHL_FUNC SealHip_ProductStats(uint64_t *fused, uint64_t *formed, uint64_t *dropped);
/* Rotations (round 6).  Evaluator_ApplyGalois / RotateVector / ComplexConjugate of a CKKS ciphertext, at the two-pass sizes and batches
 * large enough for the un-split key switch, run no permutation kernel: the key switch's own kernels read the operand's two polynomials
 * through the automorphism's index map (util/galois.cpp:18-51 folded into evaluator.cpp:2561-2867), and the result's second polynomial -
 * zero before the key switch - is neither written nor read.  Same words.  Counters for tests: rotations that took that path / that ran
 * the permutation kernels. */
SHL_FUNC SealHip_GaloisStats(uint64_t *gathered, uint64_t *permuted);
/* sample_poly_uniform on the device (seeded streams, fresh encryptions) since the library was loaded: polynomials expanded, rejected
 * words the host replaced in the reference's order, nanoseconds of that host walk, nanoseconds of the expansion calls altogether */
SHL_FUNC SealHip_XofStats(uint64_t *polynomials, uint64_t *replaced_words, uint64_t *host_walk_ns, uint64_t *total_ns);
/* stream and device memory helpers for bindings without their own runtime (a PyTorch / HIP caller passes its own streams) */
/* one process per GPU: select the calling thread's device before creating a SEALContext (a PyTorch caller uses
 * torch.cuda.set_device instead) */
SHL_FUNC shl_device_count(int *count);
SHL_FUNC shl_set_device(int device);
SHL_FUNC shl_stream_create(bool non_blocking, void **hip_stream);
SHL_FUNC shl_stream_destroy(void *hip_stream);
SHL_FUNC shl_malloc(uint64_t bytes, void **device_ptr);
SHL_FUNC shl_free(void *device_ptr);
SHL_FUNC shl_memcpy_h2d(void *device_dst, const void *host_src, uint64_t bytes);
/* KeyGenerator (native/src/seal/c/keygenerator.h:16-36; seal::KeyGenerator, native/src/seal/keygenerator.cpp): secret key, public
 * key, RelinKeys and GaloisKeys generated in HBM with the reference's algorithm and randomness (device samplers over the
 * reference's BLAKE2Xb streams).  seed8 = 8 words for the reference's seeded factory (Blake2xbPRNGFactory(seed): reproducible,
 * word-for-word the reference's keys) or NULL for operating-system entropy.
 * !! seed8 != NULL IS INSECURE AND FOR PARITY TESTS ONLY.  Like the reference's seeded Blake2xbPRNGFactory (a test device there
 * too), every sampling call restarts from the same seed: the secret key, every key-switching digit and every encryption draw
 * the same (a, e), so differences of key components reveal s^2 / the rotated s, and the public seed written into saved streams
 * is the head of the stream that sampled the secret key.  Production callers pass NULL.  The same holds for Encryptor_SetSeed. !!
 * Differences from sealc: destinations are objects
 * the caller created (SecretKey_Create / PublicKey_Create / KSwitchKeys_Create1) rather than returned handles; the save_seed
 * forms write the stream directly (the *Save functions below).  KeyGenerator_KeyToHost regenerates one key in the
 * reference's layout [digit][2][L][N] into host memory (galois_elt 0 = the relinearization key); SecretKey_Get / PublicKey_Get
 * copy SecretKey::data() / PublicKey::data() to the host. */
SHL_FUNC KeyGenerator_Create1(void *context, const uint64_t *seed8, void **key_generator);
SHL_FUNC KeyGenerator_Create2(void *context, void *secret_key, const uint64_t *seed8, void **key_generator);
SHL_FUNC KeyGenerator_Destroy(void *thisptr);
SHL_FUNC KeyGenerator_SecretKey(void *thisptr, void *secret_key);
SHL_FUNC KeyGenerator_CreatePublicKey(void *thisptr, void *public_key);
SHL_FUNC KeyGenerator_CreateRelinKeys(void *thisptr, void *relin_keys);
SHL_FUNC KeyGenerator_CreateGaloisKeysFromElts(void *thisptr, uint64_t count, const uint32_t *galois_elts, void *galois_keys);
SHL_FUNC KeyGenerator_CreateGaloisKeysFromSteps(void *thisptr, uint64_t count, const int *steps, void *galois_keys);
SHL_FUNC KeyGenerator_CreateGaloisKeysAll(void *thisptr, void *galois_keys);
/* the save_seed = true forms, saved: Serializable<RelinKeys> / Serializable<GaloisKeys>::save(compr_mode none) - every digit as its seeded
 * ciphertext (c_0 + the seed of c_1), half the bytes of the full keys; byte for byte the reference's stream under its seeded factory */
SHL_FUNC KeyGenerator_SeededSaveSize(void *thisptr, bool galois, uint64_t key_count, int64_t *result);
SHL_FUNC KeyGenerator_CreateRelinKeysSave(void *thisptr, uint8_t *outptr, uint64_t size, int64_t *out_bytes);
SHL_FUNC KeyGenerator_CreateGaloisKeysFromEltsSave(void *thisptr, uint64_t count, const uint32_t *galois_elts, uint8_t *outptr, uint64_t size,
                                                   int64_t *out_bytes);
SHL_FUNC KeyGenerator_KeyToHost(void *thisptr, uint32_t galois_elt, uint64_t *host_words, uint64_t capacity_words);
SHL_FUNC SecretKey_Get(void *thisptr, uint64_t *host_words);
SHL_FUNC PublicKey_Get(void *thisptr, uint64_t *host_words);
SHL_FUNC shl_memcpy_d2h(void *host_dst, const void *device_src, uint64_t bytes);
SHL_FUNC shl_device_synchronize(void);
/* HIP-event timing on the library's stream (bench.py measures kernels where they are launched) */
SHL_FUNC shl_timer_create(void **timer);
SHL_FUNC shl_timer_destroy(void *timer);
SHL_FUNC shl_timer_start(void *timer, void *stream);
SHL_FUNC shl_timer_stop(void *timer, void *stream, float *milliseconds); /* synchronises on the stop event */

#ifdef __cplusplus
}
#endif
/* library extensions declared in headers of their own */
#include "sealhip_galois_set.h"
#endif /* SEALHIP_H */
