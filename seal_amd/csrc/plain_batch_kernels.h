// Kernels of the Evaluator's per-item plaintext operands (evaluator.h: add_plain_device / sub_plain_device / multiply_plain_device):
// plaintext b is applied to item b of a batch ciphertext, where poly_kernels.h's k_dyadic_plain / k_addsub_plain / k_bfv_addsub_plain
// apply one plaintext to every item.  Element-wise and HBM-streaming like encrypt_kernels.h: one thread moves two adjacent words per
// operand with one 16-byte access, the grid is flat (one thread per pair, no loop over the grid), and every operand except the small
// per-level constant tables carries the non-temporal hint - each word is read once or written once.
// Layouts: a ciphertext plane is [batch][K][N]; a launch covers `items` consecutive items of it (the caller offsets the pointers by
// the chunk's first item); NTT-form plaintexts are [items][K][N], coefficient-form ones [items][N] modulo t.
// Source and result are separate arguments and may be the same words (in place): a thread reads its pair before it writes it.  The
// monomial product is the exception (it permutes): its result must not be its source.
// Every result is the canonical residue of an exactly specified integer, hence the words of the per-object forms.
#pragma once
#include "encrypt_kernels.h"

namespace sealhip
{
    // r[p][b][k] = a[p][b][k] .* pl[b][k], p < size (multiply_plain_ntt, evaluator.cpp:2157-2194, with item b's plaintext).  Plane p of
    // the source is a + p * a_stride, of the result r + p * r_stride.  A thread keeps its two plaintext words in registers over the
    // `size` planes: the plaintext plane crosses HBM once.
    hipError_t k_dyadic_plain_batch(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride,
                                    unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // r[b][k] = a[b][k] (+/-) pl[b][k] over one plane (op 0 add, 1 sub): CKKS / BGV add_plain, sub_plain with item b's plaintext
    hipError_t k_addsub_plain_batch(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, uint64_t *r, int op, unsigned n_log, unsigned K,
                                    unsigned items, hipStream_t s);
    // BFV add_plain / sub_plain: r[b][k][j] = a[b][k][j] (+/-) scaled(m[b][j]) - multiply_add/sub_plain_with_scaling_variant
    // (util/scalingvariant.cpp:70-175) with item b's coefficients; the scaling is the device function k_encrypt_bfv_finish adds with
    hipError_t k_bfv_addsub_plain_batch(const ModDesc *mods, const BfvPlainConst &pc, const uint64_t *m, const uint64_t *a, uint64_t *r, int op,
                                        unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // stats[b] = { nonzero_coeff_count, significant_coeff_count, the coefficient at significant_coeff_count - 1 (0 if none) } of
    // m[b][0..N) (plaintext.h:371-399) - k_plain_stats for every item, one workgroup per item: decides the monomial branch of
    // multiply_plain_normal (evaluator.cpp:2051-2095) for the whole batch with one launch
    hipError_t k_plain_stats_batch(const uint64_t *m, uint64_t *stats, unsigned n_log, unsigned items, hipStream_t s);
    // negacyclic_multiply_poly_mono_coeffmod (util/polyarithsmallmod.cpp:286-334) for the items whose stats say "monomial"
    // (stats[b][0] == 1); the others are left alone.  out[p][b][k] = in[p][b][k] * (scalar_k x^e), e = stats[b][1] - 1 and, with
    // c = stats[b][2], scalar_k = c mod q_k - plus inc[k] = (Q - t) mod q_k when c >= threshold and inc != null (null: the level has
    // the fast plain lift, where the reference multiplies by the raw coefficient; Evaluator::mul_plain_monomial).  out != in.
    hipError_t k_negacyclic_mul_mono_batch(const ModDesc *mods, const uint64_t *stats, uint64_t threshold, const uint64_t *inc,
                                           const uint64_t *in, size_t in_stride, uint64_t *out, size_t out_stride, unsigned size, unsigned n_log,
                                           unsigned K, unsigned items, hipStream_t s);
} // namespace sealhip
