// Kernels of the Evaluator's plaintext operands (add_plain / sub_plain / multiply_plain / transform_to_ntt, per object and per item
// of a device-resident batch).  ONE family: every launcher takes the plaintext with its item stride in words - item b of the batch
// meets the plaintext at pl + b * stride, and stride 0 is one plaintext shared by every item (a Plaintext handle) - and, for
// coefficient form, with coeff_count, the number of words the plaintext holds (N for [batch][N] buffers, Plaintext::coeff_count()
// for a handle).  Coefficients at or beyond coeff_count are zero and are never read.
// Element-wise and HBM-streaming like encrypt_kernels.h: one thread moves two adjacent words per operand with one 16-byte access
// (pointers and non-zero strides are 16-byte aligned), the grid is flat (one thread per pair, no loop over the grid) except the
// lift's, and every ciphertext word carries the non-temporal hint - each is read once or written once.  NTT-form plaintext words
// carry it when there is one plaintext per item; a shared plaintext is read again by every item and stays in the L2 (a compile-time
// variant of the kernel); coefficients are read once per component and never carry it.
// Layouts: a ciphertext plane is [batch][K][N]; a launch covers `items` consecutive items of it (the caller offsets the pointers by
// the chunk's first item); NTT-form plaintexts are [K][N] per item, coefficient-form ones coeff_count <= N words modulo t.
// Source and result are separate arguments and may be the same words (in place): a thread reads its pair before it writes it.  The
// monomial product is the exception (it permutes): its result must not be its source.
// Every result is the canonical residue of an exactly specified integer.
#pragma once
#include "context.h"

namespace sealhip
{
    // the constants of the BFV plaintext scaling round(m Q / t) (bfv_scaled, stream_device.h)
    struct BfvPlainConst
    {
        ModDesc t;
        uint64_t q_mod_t;
        uint64_t threshold;    // plain_upper_half_threshold = (t + 1) / 2
        const uint64_t *delta; // [K] floor(Q / t) mod q_r (LevelDev::delta_mod_q)
    };

    // r[p][b][k] = a[p][b][k] .* pl[b][k], p < size (multiply_plain_ntt, evaluator.cpp:2157-2194).  Plane p of the source is
    // a + p * a_stride, of the result r + p * r_stride.  A thread keeps its two plaintext words in registers over the `size` planes:
    // the plaintext crosses HBM once.
    hipError_t k_dyadic_plain_batch(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, size_t pl_stride, uint64_t *r,
                                    size_t r_stride, unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // r[b][k] = a[b][k] (+/-) pl[b][k] over one plane (op 0 add, 1 sub): CKKS / BGV add_plain, sub_plain
    hipError_t k_addsub_plain_batch(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, size_t pl_stride, uint64_t *r, int op,
                                    unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // BFV add_plain / sub_plain: r[b][k][j] = a[b][k][j] (+/-) scaled(m[b][j]) - multiply_add/sub_plain_with_scaling_variant
    // (util/scalingvariant.cpp:70-175); the scaling is the device function k_encrypt_bfv_finish adds with.  Beyond coeff_count the
    // words pass through.
    hipError_t k_bfv_addsub_plain_batch(const ModDesc *mods, const BfvPlainConst &pc, const uint64_t *m, size_t m_stride, size_t coeff_count,
                                        const uint64_t *a, uint64_t *r, int op, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
    // BFV / BGV: out[b][r][j] = the centred lift of m[b][j] (coefficients modulo t) to q_r (transform_to_ntt_inplace /
    // multiply_plain_normal, evaluator.cpp:2098-2125, 2243-2282): m_j mod q_r, plus inc[r] = (Q - t) mod q_r when m_j >= threshold;
    // zero beyond coeff_count.  scale_by != 1 first multiplies m[b][j] by it modulo t (BGV add_plain: the ciphertext's correction
    // factor).  out is [items][K][N] whatever the stride.
    hipError_t k_plain_lift_batch(const ModDesc *mods, const ModDesc &t, uint64_t scale_by, const uint64_t *m, size_t m_stride,
                                  size_t coeff_count, uint64_t threshold, const uint64_t *inc, uint64_t *out, unsigned n_log, unsigned K,
                                  unsigned items, hipStream_t s);
    // stats[b] = { nonzero_coeff_count, significant_coeff_count, the coefficient at significant_coeff_count - 1 (0 if none) } of
    // m[b][0..coeff_count) (plaintext.h:371-399), one workgroup per item; every word of stats[b] is written.  Decides the monomial
    // branch of multiply_plain_normal (evaluator.cpp:2051-2095) for the whole batch with one launch.
    hipError_t k_plain_stats_batch(const uint64_t *m, size_t m_stride, size_t coeff_count, uint64_t *stats, unsigned items, hipStream_t s);
    // negacyclic_multiply_poly_mono_coeffmod (util/polyarithsmallmod.cpp:286-334) for the items whose stats say "monomial"
    // (stats[b][0] == 1); the others are left alone.  Item b's stats are at stats + b * stats_stride (3, or 0 when the stats of the one
    // shared plaintext serve every item).  out[p][b][k] = in[p][b][k] * (scalar_k x^e), e = stats[b][1] - 1 and, with c = stats[b][2],
    // scalar_k = c mod q_k - plus inc[k] = (Q - t) mod q_k when c >= threshold and inc != null (null: the level has the fast plain
    // lift, where the reference multiplies by the raw coefficient).  out != in.
    hipError_t k_negacyclic_mul_mono_batch(const ModDesc *mods, const uint64_t *stats, size_t stats_stride, uint64_t threshold,
                                           const uint64_t *inc, const uint64_t *in, size_t in_stride, uint64_t *out, size_t out_stride,
                                           unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s);
} // namespace sealhip
