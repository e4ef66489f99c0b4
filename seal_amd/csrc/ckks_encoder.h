// seal::CKKSEncoder on the device (native/src/seal/ckks.h, ckks.cpp): vectors of N/2 complex (or real) numbers
// <-> NTT-form plaintexts.  Host: the index map, the complex root tables (util::ComplexRoots, croots.cpp: std::polar over an
// eighth of the circle and its symmetries - computed here with the same expressions and the same libm) and the multi-precision
// CRT constants.  Device: the FFT, the rounding / decomposition, the NTT engine, the CRT composition (ckks_kernels.h).
#pragma once
#include "ckks_kernels.h"
#include "evaluator.h"

namespace sealhip
{
    // Multi-precision CRT constants of a level, one device block of K*K + 4K words (RNSBase::initialize, rns.cpp:212-257;
    // total_coeff_modulus / upper_half_threshold, context.cpp:300-330): punct [K][K] (Q / q_j as K words) | Q [K] | (Q + 1) / 2 [K] |
    // (Q / q_j)^-1 mod q_j as K Shoup pairs.  The caller owns the block (hipFree).
    uint64_t *build_crt_constants(const Context &context, const Level &lvl);

    // The batched forms work through the batch in chunks whose scratch (the pass-to-pass vectors, and for decode the copy of the
    // words the inverse NTT runs on) stays within this many bytes; an item that needs more alone is a chunk of one.
    constexpr size_t kCkksBatchScratchBytes = size_t(256) << 20;

    class CKKSEncoder
    {
    public:
        explicit CKKSEncoder(const Context &context); // ckks.cpp:16-70
        ~CKKSEncoder();
        CKKSEncoder(const CKKSEncoder &) = delete;
        CKKSEncoder &operator=(const CKKSEncoder &) = delete;
        size_t slot_count() const { return slots_; }
        // CKKSEncoder::encode(values, parms_id, scale, destination) (ckks.h:458-680): values = count <= N/2 complex numbers as
        // (re, im) pairs, or real numbers when is_complex is false
        void encode(const double *values, size_t count, bool is_complex, const uint64_t *parms_id, double scale, Plaintext &destination) const;
        // CKKSEncoder::encode(double value, ...) / encode(int64_t value, ...) (ckks.cpp:72-250): the value in every slot = a
        // constant polynomial, whose NTT form is that constant in every position
        void encode_value(double value, const uint64_t *parms_id, double scale, Plaintext &destination) const;
        void encode_integer(int64_t value, const uint64_t *parms_id, Plaintext &destination) const;
        // `count` such values as scalars (CKKSEncoder_EncodeScalars / _EncodeIntegerScalars, include/sealhip.h): host values in,
        // [count][K] words in the caller's device buffer out - word k of scalar i is what encode_value / encode_integer put at every
        // coefficient of prime k, and their refusals are passed on with the first failing index; a failed call writes nothing
        void encode_scalars(size_t count, const double *values, const uint64_t *parms_id, double scale, uint64_t *device_words) const;
        void encode_integer_scalars(size_t count, const int64_t *values, const uint64_t *parms_id, uint64_t *device_words) const;
        // CKKSEncoder::decode (ckks.h:683-789): N/2 complex numbers as (re, im) pairs, or their real parts
        void decode(const Plaintext &plain, double *values, bool want_complex) const;
        // whole batches in device memory (CKKSEncoder_EncodeDevice / _DecodeDevice, include/sealhip.h): encode writes [batch][K][N]
        // NTT-form words, item b = encode(values_b, parms_id, scale).data(); decode reads such words and writes [batch][N/2] reals
        // or [batch][N/2][2] (re, im).  Null stream; both return after the work is done.
        void encode_device(const double *values, size_t value_count, size_t batch, bool is_complex, const uint64_t *parms_id, double scale,
                           uint64_t *words) const;
        void decode_device(const uint64_t *words, size_t batch, const uint64_t *parms_id, double scale, bool want_complex, double *values) const;

    private:
        const Level &value_level(const uint64_t *parms_id, double scale) const;
        void value_residues(double value, const Level &lvl, double scale, uint64_t *residues) const;
        void integer_residues(int64_t value, const Level &lvl, uint64_t *residues) const;
        template <class Residues>
        void upload_scalars(size_t count, const void *values, const Level &lvl, uint64_t *device_words, Residues residues) const;
        void fill_constant(const Level &lvl, const std::vector<uint64_t> &residues, double scale, Plaintext &destination) const;
        struct LevelConst
        {
            uint64_t *dev = nullptr; // punct [K][K] | q_words [K] | half_words [K] | inv_punct [K] Shoup pairs
            double coeff_limit = 0;  // the largest |coefficient| encode_internal accepts at this level (see coeff_limit())
        };
        const LevelConst &level_const(const Level &lvl) const;
        const Level &encode_level(const uint64_t *parms_id, double scale, size_t value_count, bool have_values) const;
        const Level &decode_level(const uint64_t *parms_id, double scale) const;
        void encode_batch(const double *values, size_t value_count, size_t batch, bool is_complex, const Level &lvl, double scale,
                          uint64_t *words) const;
        void decode_batch(const uint64_t *words, size_t batch, const Level &lvl, double scale, bool want_complex, double *values) const;
        unsigned block_log() const;
        size_t chunk_items(size_t item_words) const;
        const Context &context_;
        size_t slots_;
        uint32_t *inv_map_ = nullptr;
        double2 *roots_ = nullptr, *inv_roots_ = nullptr;
        mutable std::mutex mu_;
        mutable std::map<size_t, LevelConst> consts_;
    };
} // namespace sealhip
