// See encrypt_kernels.h.  One thread = two adjacent words of every operand: N >= 2 is a power of two and rows are 16-byte aligned,
// so a pair lies inside one row down to N = 2 (tests: the ring sizes 2 and 8 of test_encrypt_at_sampling_thresholds).
#include "stream_device.h"

namespace sealhip
{
    namespace
    {
        constexpr unsigned kBlock = 256;
        inline unsigned grid_for(size_t work)
        {
            size_t b = (work + kBlock - 1) / kBlock;
            if (b > 2048)
                b = 2048;
            if (b == 0)
                b = 1;
            return (unsigned)b;
        }
        __device__ __forceinline__ uint64_t lift_small(int v, uint64_t q)
        {
            return v < 0 ? q - (uint64_t)(-v) : (uint64_t)v;
        }

        // pairs = polys * items * K * N / 2
        __global__ void __launch_bounds__(kBlock) expand_small_batch_kernel(
            const ModDesc *mods, const int8_t *small, size_t small_stride, uint64_t *dst, size_t poly_stride, size_t pairs, unsigned n_log,
            unsigned K, unsigned items)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x; t < pairs; t += (size_t)gridDim.x * kBlock)
            {
                const size_t i = 2 * t, j = i & nmask;
                const size_t row = i >> n_log; // (p * items + b) * K + r
                const unsigned r = (unsigned)(row % K);
                const size_t pb = row / K, b = pb % items, p = pb / items;
                const int8_t *src = small + b * small_stride + (p << n_log) + j;
                const uint64_t q = mods[r].q;
                st2_nt(dst + p * poly_stride + (((b * K + r) << n_log) + j), lift_small(src[0], q), lift_small(src[1], q));
            }
        }

        // pairs = items * K * N / 2
        template <bool PRODUCT_ONLY>
        __global__ void __launch_bounds__(kBlock) encrypt_sym_tail_kernel(
            const ModDesc *mods, const uint64_t *sk, const uint64_t *a, uint64_t *c0, const uint64_t *m, uint64_t noise_factor, size_t pairs,
            unsigned n_log, unsigned K)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x; t < pairs; t += (size_t)gridDim.x * kBlock)
            {
                const size_t i = 2 * t;
                const unsigned r = (unsigned)((i >> n_log) % K);
                const ModDesc md = mods[r];
                uint64_t a0, a1, s0, s1;
                ld2<true>(a + i, a0, a1);
                ld2<false>(sk + (((size_t)r << n_log) + (i & nmask)), s0, s1); // shared by every item: stays in the L2
                uint64_t v0 = mul_mod(a0, s0, md), v1 = mul_mod(a1, s1, md);
                if (!PRODUCT_ONLY)
                {
                    uint64_t e0, e1;
                    ld2<true>(c0 + i, e0, e1);
                    if (noise_factor != 1)
                    {
                        const uint64_t f = barrett64(noise_factor, md);
                        e0 = mul_mod(e0, f, md);
                        e1 = mul_mod(e1, f, md);
                    }
                    v0 = neg_mod(add_mod(v0, e0, md.q), md.q);
                    v1 = neg_mod(add_mod(v1, e1, md.q), md.q);
                    if (m)
                    {
                        uint64_t m0, m1;
                        ld2<true>(m + i, m0, m1);
                        v0 = add_mod(v0, m0, md.q);
                        v1 = add_mod(v1, m1, md.q);
                    }
                }
                st2_nt(c0 + i, v0, v1);
            }
        }

        template <bool PRODUCT_ONLY>
        __global__ void __launch_bounds__(kBlock) encrypt_pk_tail_kernel(
            const ModDesc *mods, const uint64_t *pk, size_t pk_stride, const uint64_t *u, uint64_t *c, size_t plane_stride, uint64_t noise_factor,
            size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x; t < pairs; t += (size_t)gridDim.x * kBlock)
            {
                const size_t i = 2 * t;
                const unsigned r = (unsigned)((i >> n_log) % K);
                const ModDesc md = mods[r];
                const size_t kj = ((size_t)r << n_log) + (i & nmask);
                uint64_t u0, u1;
                ld2<true>(u + i, u0, u1);
                const uint64_t f = noise_factor != 1 ? barrett64(noise_factor, md) : 1;
#pragma unroll
                for (unsigned p = 0; p < 2; p++)
                {
                    uint64_t k0, k1;
                    ld2<false>(pk + p * pk_stride + kj, k0, k1); // shared by every item: stays in the L2
                    uint64_t v0 = mul_mod(u0, k0, md), v1 = mul_mod(u1, k1, md);
                    uint64_t *cp = c + p * plane_stride + i;
                    if (!PRODUCT_ONLY)
                    {
                        uint64_t e0, e1;
                        ld2<true>(cp, e0, e1);
                        if (noise_factor != 1)
                        {
                            e0 = mul_mod(e0, f, md);
                            e1 = mul_mod(e1, f, md);
                        }
                        v0 = add_mod(v0, e0, md.q);
                        v1 = add_mod(v1, e1, md.q);
                    }
                    st2_nt(cp, v0, v1);
                }
            }
        }

        // pairs = planes * items * K * N / 2
        __global__ void __launch_bounds__(kBlock) encrypt_bfv_finish_kernel(
            const ModDesc *mods, BfvPlainConst pc, const int8_t *small, size_t small_stride, const uint64_t *m, uint64_t *c, size_t plane_stride,
            size_t pairs, bool negate, unsigned n_log, unsigned K, unsigned items)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x; t < pairs; t += (size_t)gridDim.x * kBlock)
            {
                const size_t i = 2 * t, j = i & nmask;
                const size_t row = i >> n_log; // (p * items + b) * K + r
                const unsigned r = (unsigned)(row % K);
                const size_t pb = row / K, b = pb % items, p = pb / items;
                const ModDesc md = mods[r];
                uint64_t *cp = c + p * plane_stride + (((b * K + r) << n_log) + j);
                uint64_t v0, v1;
                ld2<true>(cp, v0, v1);
                if (small)
                {
                    const int8_t *e = small + b * small_stride + (p << n_log) + j;
                    v0 = add_mod(v0, lift_small(e[0], md.q), md.q);
                    v1 = add_mod(v1, lift_small(e[1], md.q), md.q);
                }
                if (negate)
                {
                    v0 = neg_mod(v0, md.q);
                    v1 = neg_mod(v1, md.q);
                }
                if (m && p == 0)
                {
                    uint64_t m0, m1;
                    ld2<false>(m + (b << n_log) + j, m0, m1); // read once per component: K times
                    const uint64_t delta = pc.delta[r];
                    v0 = add_mod(v0, bfv_scaled(m0, pc, delta, md), md.q);
                    v1 = add_mod(v1, bfv_scaled(m1, pc, delta, md), md.q);
                }
                st2_nt(cp, v0, v1);
            }
        }
    } // namespace

    hipError_t k_expand_small_batch(const ModDesc *mods, const int8_t *small, size_t small_stride, uint64_t *dst, size_t poly_stride,
                                    unsigned n_log, unsigned K, unsigned polys, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)polys * items * K) << n_log) / 2;
        if (!pairs)
            return hipSuccess;
        hipLaunchKernelGGL(expand_small_batch_kernel, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, small, small_stride, dst, poly_stride, pairs,
                           n_log, K, items);
        return hipGetLastError();
    }
    hipError_t k_encrypt_sym_tail(const ModDesc *mods, const uint64_t *sk, const uint64_t *a, uint64_t *c0, const uint64_t *m,
                                  uint64_t noise_factor, bool product_only, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        if (!pairs)
            return hipSuccess;
        if (product_only)
            hipLaunchKernelGGL(encrypt_sym_tail_kernel<true>, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, sk, a, c0, m, noise_factor, pairs,
                               n_log, K);
        else
            hipLaunchKernelGGL(encrypt_sym_tail_kernel<false>, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, sk, a, c0, m, noise_factor, pairs,
                               n_log, K);
        return hipGetLastError();
    }
    hipError_t k_encrypt_pk_tail(const ModDesc *mods, const uint64_t *pk, size_t pk_stride, const uint64_t *u, uint64_t *c, size_t plane_stride,
                                 uint64_t noise_factor, bool product_only, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        if (!pairs)
            return hipSuccess;
        if (product_only)
            hipLaunchKernelGGL(encrypt_pk_tail_kernel<true>, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, pk, pk_stride, u, c, plane_stride,
                               noise_factor, pairs, n_log, K);
        else
            hipLaunchKernelGGL(encrypt_pk_tail_kernel<false>, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, pk, pk_stride, u, c, plane_stride,
                               noise_factor, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_encrypt_bfv_finish(const ModDesc *mods, const BfvPlainConst &pc, const int8_t *small, size_t small_stride, const uint64_t *m,
                                    uint64_t *c, size_t plane_stride, unsigned planes, bool negate, unsigned n_log, unsigned K, unsigned items,
                                    hipStream_t s)
    {
        const size_t pairs = (((size_t)planes * items * K) << n_log) / 2;
        if (!pairs)
            return hipSuccess;
        hipLaunchKernelGGL(encrypt_bfv_finish_kernel, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, pc, small, small_stride, m, c, plane_stride,
                           pairs, negate, n_log, K, items);
        return hipGetLastError();
    }
} // namespace sealhip
