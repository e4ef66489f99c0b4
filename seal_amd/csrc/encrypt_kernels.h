// Kernels of the Encryptor's two bodies (decryptor.h: symmetric / asymmetric): `items` independent fresh ciphertexts per launch,
// every item with its own randomness and its own plaintext; the per-object forms and the KeyGenerator run them with items = 1.
// Element-wise and HBM-streaming: each thread moves two adjacent words per operand with one 16-byte access; operands that are read
// once and results that are written once carry the non-temporal hint, so that what the whole batch shares (s, the public key)
// stays in the L2.  N >= 2 (the Context's constructor enforces it) and rows of N * 8 bytes in 16-byte aligned slabs: a pair never
// straddles two rows and every access is aligned, down to N = 2 (one pair per row).
// Layouts: a ciphertext plane chunk is [items][K][N]; keys are [L][N] at the key level (component r of a level = prime r);
// the small polynomials are signed bytes, item b at small + b * small_stride.
// Every result is the canonical residue of an exactly specified integer, whatever the order of the additions.
#pragma once
#include "plain_batch_kernels.h" // BfvPlainConst; the per-item lift of the BGV plaintexts (k_plain_lift_batch)

namespace sealhip
{
    // out[p][b][r][j] = small[b][p * N + j] lifted to [0, q_r), p < polys; plane p of the output starts at dst + p * poly_stride
    hipError_t k_expand_small_batch(const ModDesc *mods, const int8_t *small, size_t small_stride, uint64_t *dst, size_t poly_stride,
                                    unsigned n_log, unsigned K, unsigned polys, unsigned items, hipStream_t s);
    // Symmetric tail (util/rlwe.cpp:357-381 and the plaintext addition of Encryptor::encrypt_internal) in one pass.
    //   product_only == false (CKKS, BGV; everything in NTT form): c0 holds the transformed noise e^ and becomes
    //     m - (a s + noise_factor e^) mod q_r;  m = [items][K][N] words or null (zero), noise_factor = t (BGV) or 1
    //   product_only == true (BFV, whose tail follows the inverse transform: k_encrypt_bfv_finish): c0 = a s
    hipError_t k_encrypt_sym_tail(const ModDesc *mods, const uint64_t *sk, const uint64_t *a, uint64_t *c0, const uint64_t *m,
                                  uint64_t noise_factor, bool product_only, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // Public-key tail (util/rlwe.cpp:226-262) over both planes: c_j = pk_j u^ [+ noise_factor e^_j, held by c_j; not when
    // product_only], j = 0, 1.  pk = [2][L][N] (pk_stride = L * N words), u = [items][K][N], c_1 = c_0 + plane_stride.
    hipError_t k_encrypt_pk_tail(const ModDesc *mods, const uint64_t *pk, size_t pk_stride, const uint64_t *u, uint64_t *c, size_t plane_stride,
                                 uint64_t noise_factor, bool product_only, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // BFV, coefficient form, `planes` planes of [items][K][N] (plane_stride apart):
    //   c_p <- c_p + e_p            e_p[b][j] = small[b][p * N + j]; small == null: no noise
    //   c_p <- -c_p                 when negate (the symmetric form)
    //   c_0 <- c_0 + scaled(m_b)    m = [items][N] coefficients modulo t or null: multiply_add_plain_with_scaling_variant
    //                               (util/scalingvariant.cpp:70-115), what k_bfv_addsub_plain_batch adds
    hipError_t k_encrypt_bfv_finish(const ModDesc *mods, const BfvPlainConst &pc, const int8_t *small, size_t small_stride, const uint64_t *m,
                                    uint64_t *c, size_t plane_stride, unsigned planes, bool negate, unsigned n_log, unsigned K, unsigned items,
                                    hipStream_t s);
} // namespace sealhip
