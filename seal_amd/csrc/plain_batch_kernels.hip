// See plain_batch_kernels.h.  One thread = two adjacent words of every operand (N is even, rows are 16-byte aligned); flat grids
// except the lift's.
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
        inline unsigned grid_for(size_t work)
        {
            size_t b = (work + kBlock - 1) / kBlock;
            if (b > 2048)
                b = 2048;
            if (b == 0)
                b = 1;
            return (unsigned)b;
        }

        // coefficients j and j + 1 (j even) of a plaintext that holds `count` words: those at or beyond count are zero and are not read
        __device__ __forceinline__ void ld_coeffs(const uint64_t *m, size_t j, size_t count, uint64_t &m0, uint64_t &m1)
        {
            m0 = m1 = 0;
            if (j + 1 < count)
                ld2<false>(m + j, m0, m1); // read once per component, K times: through the L2
            else if (j < count)
                m0 = m[j];
        }

        // pairs = items * K * N / 2; SIZE = the number of planes when it is 2 or 3, 0 = `size`; NT_PLAIN: the plaintext words carry
        // the non-temporal hint (one plaintext per item: read once), not when every item reads the same ones
        template <unsigned SIZE, bool NT_PLAIN>
        __global__ void __launch_bounds__(kBlock) dyadic_plain_batch_kernel(
            const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, size_t pl_stride, uint64_t *r, size_t r_stride,
            unsigned size, size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w, row = i >> n_log, b = row / K; // row = b * K + k
            const ModDesc md = mods[row - b * K];
            uint64_t p0, p1;
            ld2<NT_PLAIN>(pl + b * pl_stride + (i - b * ((size_t)K << n_log)), p0, p1);
            const unsigned planes = SIZE ? SIZE : size; // (a constant trip count unrolls)
            for (unsigned p = 0; p < planes; p++)
            {
                uint64_t a0, a1;
                ld2<true>(a + p * a_stride + i, a0, a1);
                st2_nt(r + p * r_stride + i, mul_mod(a0, p0, md), mul_mod(a1, p1, md));
            }
        }

        // pairs = items * K * N / 2
        template <bool NT_PLAIN>
        __global__ void __launch_bounds__(kBlock) addsub_plain_batch_kernel(
            const ModDesc *mods, const uint64_t *a, const uint64_t *pl, size_t pl_stride, uint64_t *r, int op, size_t pairs, unsigned n_log,
            unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w, row = i >> n_log, b = row / K; // row = b * K + k
            const uint64_t q = mods[row - b * K].q;
            uint64_t a0, a1, p0, p1;
            ld2<true>(a + i, a0, a1);
            ld2<NT_PLAIN>(pl + b * pl_stride + (i - b * ((size_t)K << n_log)), p0, p1);
            if (op)
                st2_nt(r + i, sub_mod(a0, p0, q), sub_mod(a1, p1, q));
            else
                st2_nt(r + i, add_mod(a0, p0, q), add_mod(a1, p1, q));
        }

        // pairs = items * K * N / 2
        __global__ void __launch_bounds__(kBlock) bfv_addsub_plain_batch_kernel(
            const ModDesc *mods, BfvPlainConst pc, const uint64_t *m, size_t m_stride, size_t coeff_count, const uint64_t *a, uint64_t *r, int op,
            size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t i = 2 * w, row = i >> n_log, b = row / K, j = i & ((size_t(1) << n_log) - 1); // row = b * K + k
            if (j >= coeff_count && r == a)
                return; // nothing is added: the words stay
            uint64_t a0, a1, m0, m1;
            ld2<true>(a + i, a0, a1);
            if (j >= coeff_count)
            {
                st2_nt(r + i, a0, a1);
                return;
            }
            const unsigned k = (unsigned)(row - b * K);
            const ModDesc md = mods[k];
            ld_coeffs(m + b * m_stride, j, coeff_count, m0, m1);
            const uint64_t delta = pc.delta[k];
            const uint64_t s0 = bfv_scaled(m0, pc, delta, md), s1 = bfv_scaled(m1, pc, delta, md); // scaled(0) = 0
            if (op)
                st2_nt(r + i, sub_mod(a0, s0, md.q), sub_mod(a1, s1, md.q));
            else
                st2_nt(r + i, add_mod(a0, s0, md.q), add_mod(a1, s1, md.q));
        }

        // pairs = items * K * N / 2
        __global__ void __launch_bounds__(kBlock) plain_lift_batch_kernel(
            const ModDesc *mods, ModDesc t, uint64_t scale_by, const uint64_t *m, size_t m_stride, size_t coeff_count, uint64_t threshold,
            const uint64_t *inc, uint64_t *out, size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x; w < pairs; w += (size_t)gridDim.x * kBlock)
            {
                const size_t i = 2 * w, row = i >> n_log, b = row / K; // row = b * K + r
                const unsigned r = (unsigned)(row - b * K);
                const ModDesc md = mods[r];
                uint64_t m0, m1;
                ld_coeffs(m + b * m_stride, i & nmask, coeff_count, m0, m1);
                if (scale_by != 1)
                {
                    m0 = mul_mod(m0, scale_by, t);
                    m1 = mul_mod(m1, scale_by, t);
                }
                uint64_t v0 = barrett64(m0, md), v1 = barrett64(m1, md);
                const uint64_t up = inc[r];
                if (m0 >= threshold)
                    v0 = add_mod(v0, up, md.q);
                if (m1 >= threshold)
                    v1 = add_mod(v1, up, md.q);
                st2_nt(out + i, v0, v1);
            }
        }

        // one workgroup per item
        __global__ void __launch_bounds__(kBlock) plain_stats_batch_kernel(const uint64_t *m, size_t m_stride, size_t coeff_count, uint64_t *stats)
        {
            __shared__ unsigned long long s_nz[kBlock], s_last[kBlock];
            const uint64_t *mb = m + blockIdx.x * m_stride;
            const size_t pairs = (coeff_count + 1) / 2;
            unsigned long long nz = 0, last = 0; // last = index of the last nonzero coefficient + 1
            for (size_t w = threadIdx.x; w < pairs; w += kBlock)
            {
                uint64_t m0, m1;
                ld_coeffs(mb, 2 * w, coeff_count, m0, m1); // the lift or the scaling reads the coefficients again
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
            const ModDesc *mods, const uint64_t *stats, size_t stats_stride, uint64_t threshold, const uint64_t *inc, const uint64_t *in,
            size_t in_stride, uint64_t *out, size_t out_stride, unsigned size, size_t pairs, unsigned n_log, unsigned K)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= pairs)
                return;
            const size_t N = size_t(1) << n_log, i = 2 * w, row = i >> n_log; // b * K + k
            const uint64_t *st = stats + stats_stride * (row / K);
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

        template <bool NT_PLAIN>
        void launch_dyadic(unsigned blocks, hipStream_t s, const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl,
                           size_t pl_stride, uint64_t *r, size_t r_stride, unsigned size, size_t pairs, unsigned n_log, unsigned K)
        {
            if (size == 2)
                hipLaunchKernelGGL((dyadic_plain_batch_kernel<2, NT_PLAIN>), dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, pl_stride, r,
                                   r_stride, size, pairs, n_log, K);
            else if (size == 3)
                hipLaunchKernelGGL((dyadic_plain_batch_kernel<3, NT_PLAIN>), dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, pl_stride, r,
                                   r_stride, size, pairs, n_log, K);
            else
                hipLaunchKernelGGL((dyadic_plain_batch_kernel<0, NT_PLAIN>), dim3(blocks), dim3(kBlock), 0, s, mods, a, a_stride, pl, pl_stride, r,
                                   r_stride, size, pairs, n_log, K);
        }
    } // namespace

    hipError_t k_dyadic_plain_batch(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, size_t pl_stride, uint64_t *r,
                                    size_t r_stride, unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs || !size)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        if (pl_stride)
            launch_dyadic<true>(blocks, s, mods, a, a_stride, pl, pl_stride, r, r_stride, size, pairs, n_log, K);
        else
            launch_dyadic<false>(blocks, s, mods, a, a_stride, pl, pl_stride, r, r_stride, size, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_addsub_plain_batch(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, size_t pl_stride, uint64_t *r, int op,
                                    unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        if (pl_stride)
            hipLaunchKernelGGL(addsub_plain_batch_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, mods, a, pl, pl_stride, r, op, pairs, n_log, K);
        else
            hipLaunchKernelGGL(addsub_plain_batch_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, mods, a, pl, pl_stride, r, op, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_bfv_addsub_plain_batch(const ModDesc *mods, const BfvPlainConst &pc, const uint64_t *m, size_t m_stride, size_t coeff_count,
                                        const uint64_t *a, uint64_t *r, int op, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs || (!coeff_count && r == a))
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(bfv_addsub_plain_batch_kernel, dim3(blocks), dim3(kBlock), 0, s, mods, pc, m, m_stride, coeff_count, a, r, op, pairs,
                           n_log, K);
        return hipGetLastError();
    }
    hipError_t k_plain_lift_batch(const ModDesc *mods, const ModDesc &t, uint64_t scale_by, const uint64_t *m, size_t m_stride,
                                  size_t coeff_count, uint64_t threshold, const uint64_t *inc, uint64_t *out, unsigned n_log, unsigned K,
                                  unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        if (!pairs)
            return hipSuccess;
        hipLaunchKernelGGL(plain_lift_batch_kernel, dim3(grid_for(pairs)), dim3(kBlock), 0, s, mods, t, scale_by, m, m_stride, coeff_count,
                           threshold, inc, out, pairs, n_log, K);
        return hipGetLastError();
    }
    hipError_t k_plain_stats_batch(const uint64_t *m, size_t m_stride, size_t coeff_count, uint64_t *stats, unsigned items, hipStream_t s)
    {
        if (!items)
            return hipSuccess;
        hipLaunchKernelGGL(plain_stats_batch_kernel, dim3(items), dim3(kBlock), 0, s, m, m_stride, coeff_count, stats);
        return hipGetLastError();
    }
    hipError_t k_negacyclic_mul_mono_batch(const ModDesc *mods, const uint64_t *stats, size_t stats_stride, uint64_t threshold,
                                           const uint64_t *inc, const uint64_t *in, size_t in_stride, uint64_t *out, size_t out_stride,
                                           unsigned size, unsigned n_log, unsigned K, unsigned items, hipStream_t s)
    {
        const size_t pairs = (((size_t)items * K) << n_log) / 2;
        unsigned blocks;
        if (!pairs || !size)
            return hipSuccess;
        if (!flat_grid(pairs, blocks))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(negacyclic_mul_mono_batch_kernel, dim3(blocks), dim3(kBlock), 0, s, mods, stats, stats_stride, threshold, inc, in,
                           in_stride, out, out_stride, size, pairs, n_log, K);
        return hipGetLastError();
    }
} // namespace sealhip
