// See plain_batch_kernels.h.  One thread = two adjacent words of every operand (N is even, rows are 16-byte aligned); flat grids.
#include "plain_batch_kernels.h"
#include "stream_device.h"

namespace sealhip
{
    namespace
    {
        constexpr unsigned kBlock = 256;
        // one thread per pair: false when the launch would not fit the grid's x dimension
        inline bool flat_grid(size_t pairs, unsigned &blocks)
        {
            const size_t b = (pairs + kBlock - 1) / kBlock;
            blocks = (unsigned)b;
            return b <= 0x7fffffffu;
        }

        // pairs = items * K * N / 2; SIZE = the number of planes when it is 2 or 3, 0 = `size`
        template <unsigned SIZE>
        __global__ void __launch_bounds__(kBlock) dyadic_plain_batch_kernel(
            const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride, unsigned size,
            size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w;
            const ModDesc md = mods[(i >> n_log) % K];
            uint64_t p0, p1;
            ld2<true>(pl + i, p0, p1);
            const unsigned planes = SIZE ? SIZE : size; // (a constant trip count unrolls)
            for (unsigned p = 0; p < planes; p++)
            {
                uint64_t a0, a1;
                ld2<true>(a + p * a_stride + i, a0, a1);
                st2_nt(r + p * r_stride + i, mul_mod(a0, p0, md), mul_mod(a1, p1, md));
            }
        }

        // pairs = items * K * N / 2
        __global__ void __launch_bounds__(kBlock) addsub_plain_batch_kernel(
            const ModDesc *mods, const uint64_t *a, const uint64_t *pl, uint64_t *r, int op, size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w;
            const uint64_t q = mods[(i >> n_log) % K].q;
            uint64_t a0, a1, p0, p1;
            ld2<true>(a + i, a0, a1);
            ld2<true>(pl + i, p0, p1);
            if (op)
                st2_nt(r + i, sub_mod(a0, p0, q), sub_mod(a1, p1, q));
            else
                st2_nt(r + i, add_mod(a0, p0, q), add_mod(a1, p1, q));
        }

        // pairs = items * K * N / 2
        __global__ void __launch_bounds__(kBlock) bfv_addsub_plain_batch_kernel(
            const ModDesc *mods, BfvPlainConst pc, const uint64_t *m, const uint64_t *a, uint64_t *r, int op, size_t pairs, unsigned n_log,
            unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w, row = i >> n_log; // b * K + k
            const unsigned k = (unsigned)(row % K);
            const ModDesc md = mods[k];
            uint64_t a0, a1, m0, m1;
            ld2<true>(a + i, a0, a1);
            ld2<false>(m + ((row / K) << n_log) + (i & ((size_t(1) << n_log) - 1)), m0, m1); // read once per component: K times
            const uint64_t delta = pc.delta[k];
            const uint64_t s0 = bfv_scaled(m0, pc, delta, md), s1 = bfv_scaled(m1, pc, delta, md);
            if (op)
                st2_nt(r + i, sub_mod(a0, s0, md.q), sub_mod(a1, s1, md.q));
            else
                st2_nt(r + i, add_mod(a0, s0, md.q), add_mod(a1, s1, md.q));
        }

        // one workgroup per item
        __global__ void __launch_bounds__(kBlock) plain_stats_batch_kernel(const uint64_t *m, uint64_t *stats, unsigned n_log)
        {
            __shared__ unsigned long long s_nz[kBlock], s_last[kBlock];
            const uint64_t *mb = m + ((size_t)blockIdx.x << n_log);
            const size_t pairs = (size_t(1) << n_log) / 2;
            unsigned long long nz = 0, last = 0; // last = index of the last nonzero coefficient + 1
            for (size_t w = threadIdx.x; w < pairs; w += kBlock)
            {
                uint64_t m0, m1;
                ld2<false>(mb + 2 * w, m0, m1); // the lift or the scaling reads the coefficients again
                nz += (m0 != 0) + (m1 != 0);
                if (m0)
                    last = 2 * w + 1;
                if (m1)
                    last = 2 * w + 2;
            }
            s_nz[threadIdx.x] = nz;
            s_last[threadIdx.x] = last;
            __syncthreads();
            for (unsigned h = kBlock / 2; h; h /= 2)
            {
                if (threadIdx.x < h)
                {
                    s_nz[threadIdx.x] += s_nz[threadIdx.x + h];
                    if (s_last[threadIdx.x + h] > s_last[threadIdx.x])
                        s_last[threadIdx.x] = s_last[threadIdx.x + h];
                }
                __syncthreads();
            }
            if (threadIdx.x == 0)
            {
                uint64_t *st = stats + 3 * (size_t)blockIdx.x;
                st[0] = s_nz[0];
                st[1] = s_last[0];
                st[2] = s_last[0] ? mb[s_last[0] - 1] : 0;
            }
        }

        // pairs = items * K * N / 2
        __global__ void __launch_bounds__(kBlock) negacyclic_mul_mono_batch_kernel(
            const ModDesc *mods, const uint64_t *stats, uint64_t threshold, const uint64_t *inc, const uint64_t *in, size_t in_stride,
            uint64_t *out, size_t out_stride, unsigned size, size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t N = size_t(1) << n_log, i = 2 * w, row = i >> n_log; // b * K + k
            const uint64_t *st = stats + 3 * (row / K);
            if (st[0] != 1)
                return;
            const size_t e = (size_t)st[1] - 1; // < N
            const uint64_t c = st[2];
            const unsigned k = (unsigned)(row % K);
            const ModDesc md = mods[k];
            uint64_t sc = barrett64(c, md);
            if (inc && c >= threshold)
                sc = add_mod(sc, inc[k], md.q);
            // coefficients j and j + 1 go to j + e and j + e + 1 modulo N, negated where they wrap: an adjacent, aligned pair again
            // when e is even
            const size_t j = i & (N - 1), d0 = j + e, d1 = d0 + 1;
            const bool neg0 = d0 >= N, neg1 = d1 >= N;
            const size_t base = row << n_log, o0 = d0 & (N - 1), o1 = d1 & (N - 1);
            for (unsigned p = 0; p < size; p++)
            {
                uint64_t v0, v1;
                ld2<true>(in + p * in_stride + i, v0, v1);
                v0 = mul_mod(v0, sc, md);
                v1 = mul_mod(v1, sc, md);
                if (neg0)
                    v0 = neg_mod(v0, md.q);
                if (neg1)
                    v1 = neg_mod(v1, md.q);
                uint64_t *o = out + p * out_stride + base;
                if (!(e & 1))
                    st2_nt(o + o0, v0, v1);
                else
                {
                    o[o0] = v0;
                    o[o1] = v1;
                }
            }
        }
    } // namespace

    hipError_t k_dyadic_plain_batch(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride,
                                    unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs || !size)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        if (size == 2)
            hipLaunchKernelGGL(dyadic_plain_batch_kernel<2>, dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, r, r_stride, size, pairs,
                               n_log, K);
        else if (size == 3)
            hipLaunchKernelGGL(dyadic_plain_batch_kernel<3>, dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, r, r_stride, size, pairs,
                               n_log, K);
        else
            hipLaunchKernelGGL(dyadic_plain_batch_kernel<0>, dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, r, r_stride, size, pairs,
                               n_log, K);
        return hipGetLastError();
    }
    hipError_t k_addsub_plain_batch(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, uint64_t *r, int op, unsigned n_log, unsigned K,
                                    unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(addsub_plain_batch_kernel, dim3(blocks), dim3(kBlock), 0, s, mods, a, pl, r, op, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_bfv_addsub_plain_batch(const ModDesc *mods, const BfvPlainConst &pc, const uint64_t *m, const uint64_t *a, uint64_t *r, int op,
                                        unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(bfv_addsub_plain_batch_kernel, dim3(blocks), dim3(kBlock), 0, s, mods, pc, m, a, r, op, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_plain_stats_batch(const uint64_t *m, uint64_t *stats, unsigned n_log, unsigned items, hipStream_t s)
    {
        if (!items)
            return hipSuccess;
        hipLaunchKernelGGL(plain_stats_batch_kernel, dim3(items), dim3(kBlock), 0, s, m, stats, n_log);
        return hipGetLastError();
    }
    hipError_t k_negacyclic_mul_mono_batch(const ModDesc *mods, const uint64_t *stats, uint64_t threshold, const uint64_t *inc,
                                           const uint64_t *in, size_t in_stride, uint64_t *out, size_t out_stride, unsigned size, unsigned n_log,
                                           unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs || !size)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(negacyclic_mul_mono_batch_kernel, dim3(blocks), dim3(kBlock), 0, s, mods, stats, threshold, inc, in, in_stride, out,
                           out_stride, size, pairs, n_log, K);
        return hipGetLastError();
    }
} // namespace sealhip
