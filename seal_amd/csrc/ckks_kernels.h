// Kernels of the CKKS encoder (seal::CKKSEncoder, native/src/seal/ckks.h:458-789): the complex FFT of
// util::DWTHandler (dwthandler.h:94-356) in double precision, fused with the slot placement and the rounding / RNS decomposition
// of encode_internal (encode) and with the CRT composition / scaling and the slot gather of decode_internal (decode), over a
// batch of vectors.  Floating point here is the reference's own: every operation of every butterfly is the same IEEE-754 double
// operation in the same order (complex product = (ac - bd, ad + bc), no contraction), so the results are the reference's bit
// for bit; the order in which independent butterflies run is irrelevant.
//
// Pass split.  A transform of 2^n_log values is cut at block_log = min(n_log, kFftLdsLog): the stages whose gap is below
// 2^block_log pair values inside one contiguous block of 2^block_log values, which one workgroup holds in LDS (2^12 double2 =
// 64 KiB); the others (n_log - block_log <= kFftMaxColumnLog of them) pair values of one column {c + k 2^block_log}, which one
// thread holds in registers.  Encode runs the block stages first (gap 1 -> n/2), decode the column stages first (gap n/2 -> 1);
// when the whole vector fits one block it is one launch.
#pragma once
#include "context.h"

namespace sealhip
{
    constexpr unsigned kFftLdsLog = 12;      // 2^12 complex doubles = 64 KiB of LDS per workgroup
    constexpr unsigned kFftMaxColumnLog = 5; // N = 2^17: five column stages, 32 values per thread

    // encode: `items` vectors -> [items][K][N] plaintext words in coefficient form (the NTT follows on the caller's side)
    struct CkksEncodeArgs
    {
        const double *values;   // [items][value_count] reals or [items][value_count][2] (re, im)
        uint64_t value_count;   // <= N/2; slots beyond it are zero
        int is_complex;
        const uint32_t *inv_map; // coefficient position -> slot (< N/2: the value, >= N/2: the conjugate of slot - N/2)
        const double2 *inv_roots;
        const ModDesc *mods;
        unsigned K;
        double fix;         // scale / N, folded into the last stage (transform_from_rev's scalar)
        double coeff_limit; // an item fails when some |coefficient| is not <= this (NaN, infinity, too many bits)
        uint64_t *words;
        double2 *mid;       // [items][N] between the passes (unused by a one-launch transform)
        unsigned *fail;     // zeroed; atomicMax of ~(2 (item0 + item) + code) = the first failure: code 0 = a value is not finite,
                            // 1 = a coefficient too large
        unsigned item0;
        unsigned n_log, block_log;
    };
    hipError_t k_ckks_encode(const CkksEncodeArgs &a, unsigned items, hipStream_t s);

    // decode: [items][K][N] coefficient-form residues (after the inverse NTT) -> [items][N/2] reals or [items][N/2][2] (re, im)
    struct CkksDecodeArgs
    {
        const uint64_t *residues;
        const ModDesc *mods;
        // RNSBase::compose_array constants (build_crt_constants): punct = [K][K] words (Q / q_j), inv_punct = [K] Shoup pairs,
        // q_words / half_words = Q and (Q + 1) / 2 as K words
        const uint64_t *punct;
        const ShoupOp *inv_punct;
        const uint64_t *q_words, *half_words;
        double inv_scale;
        const uint32_t *inv_map;
        const double2 *roots;
        double2 *mid;
        double *out;
        int want_complex;
        unsigned K;
        unsigned n_log, block_log;
    };
    hipError_t k_ckks_decode(const CkksDecodeArgs &a, unsigned items, hipStream_t s);

    // max over the coefficients of vector b of the bit length of the centred CRT value of (m * residue): out_bits[b] (zeroed
    // beforehand) - the norm of Decryptor::invariant_noise_budget (decryptor.cpp:222-241; poly_infty_norm_coeffmod)
    hipError_t k_crt_norm_bits(const ModDesc *mods, const uint64_t *residues, const uint64_t *punct, const ShoupOp *inv_punct,
                               const uint64_t *q_words, const uint64_t *half_words, uint64_t m, unsigned *out_bits, unsigned n_log, unsigned K,
                               unsigned batch, hipStream_t s);
} // namespace sealhip
