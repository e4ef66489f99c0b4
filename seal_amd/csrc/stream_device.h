// Device-side pieces shared by the element-wise, HBM-streaming kernels of encrypt_kernels.hip and plain_batch_kernels.hip: the
// 16-byte accesses (two adjacent words per thread and per operand, with or without the non-temporal hint) and the per-coefficient
// BFV scaling of a plaintext.  Include from a .hip file only, inside nothing; everything lives in an unnamed namespace.
#pragma once
#include "plain_batch_kernels.h"

namespace sealhip
{
    namespace
    {
        // two adjacent words with one 16-byte access; NT: the non-temporal hint (read once / written once)
        template <bool NT>
        __device__ __forceinline__ void ld2(const uint64_t *p, uint64_t &a, uint64_t &b)
        {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
            const u64x2 *q = reinterpret_cast<const u64x2 *>(p);
            const u64x2 v = NT ? __builtin_nontemporal_load(q) : *q;
            a = v.x;
            b = v.y;
#else
            a = p[0];
            b = p[1];
#endif
        }
        __device__ __forceinline__ void st2(uint64_t *p, uint64_t a, uint64_t b)
        {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
            const u64x2 v = { a, b };
            *reinterpret_cast<u64x2 *>(p) = v;
#else
            p[0] = a;
            p[1] = b;
#endif
        }
        __device__ __forceinline__ void st2_nt(uint64_t *p, uint64_t a, uint64_t b)
        {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
            const u64x2 v = { a, b };
            __builtin_nontemporal_store(v, reinterpret_cast<u64x2 *>(p));
#else
            p[0] = a;
            p[1] = b;
#endif
        }

        // floor((hi:lo) / t) for a quotient below 2^64, with t's Barrett constant floor(2^128 / t)
        __device__ __forceinline__ uint64_t div128_by(uint64_t lo, uint64_t hi, const ModDesc &t)
        {
            uint64_t t1 = mul_hi64(lo, t.ratio_lo);
            uint64_t a_lo, a_hi, b_lo, b_hi;
            mul_wide(lo, t.ratio_hi, a_lo, a_hi);
            mul_wide(hi, t.ratio_lo, b_lo, b_hi);
            uint64_t mid = t1 + a_lo;
            uint64_t c = mid < t1;
            uint64_t mid2 = mid + b_lo;
            c += mid2 < mid;
            uint64_t qest = hi * t.ratio_hi + a_hi + b_hi + c; // low by at most 2
            uint64_t r = lo - qest * t.q;
            while (r >= t.q)
            {
                r -= t.q;
                qest++;
            }
            return qest;
        }
        // round(m * Q / t) mod q_r as multiply_add_plain_with_scaling_variant forms it: m * floor(Q / t) + floor((m * (Q mod t) + (t + 1) / 2) / t)
        __device__ __forceinline__ uint64_t bfv_scaled(uint64_t mv, const BfvPlainConst &pc, uint64_t delta, const ModDesc &md)
        {
            uint64_t lo, hi;
            mul_wide(mv, pc.q_mod_t, lo, hi);
            lo += pc.threshold;
            hi += lo < pc.threshold;
            const uint64_t fix = div128_by(lo, hi, pc.t);
            return add_mod(mul_mod(mv, delta, md), barrett64(fix, md), md.q);
        }
    } // namespace
} // namespace sealhip
