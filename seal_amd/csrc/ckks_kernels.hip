// See ckks_kernels.h.
#include "ckks_kernels.h"
#include <algorithm>
#include <cmath>

namespace sealhip
{
    namespace
    {
        constexpr unsigned kBlock = 256;
        inline unsigned grid_for(size_t work)
        {
            size_t b = (work + kBlock - 1) / kBlock;
            if (b > 4096)
                b = 4096;
            if (b == 0)
                b = 1;
            return (unsigned)b;
        }
        // std::complex<double> operator* as GCC evaluates it without -ffast-math for finite operands
        __device__ __forceinline__ double2 cmul(double2 a, double2 b)
        {
            return double2{ a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x };
        }
        __device__ __forceinline__ double2 cadd(double2 a, double2 b)
        {
            return double2{ a.x + b.x, a.y + b.y };
        }
        __device__ __forceinline__ double2 csubc(double2 a, double2 b)
        {
            return double2{ a.x - b.x, a.y - b.y };
        }
        // transform_from_rev's butterfly at a gap: (x, y) <- (x + y, (x - y) r); the last stage folds the scalar in:
        // x <- (x + y) s, y <- (x - y) (r s)  (dwthandler.h:322-354, mul_root_scalar / mul_scalar)
        __device__ __forceinline__ void gs_butterfly(double2 &x, double2 &y, double2 r)
        {
            const double2 u = x, v = y;
            x = cadd(u, v);
            y = cmul(csubc(u, v), r);
        }
        __device__ __forceinline__ void gs_butterfly_scaled(double2 &x, double2 &y, double2 r, double sc)
        {
            const double2 u = x, v = y;
            const double2 scaled_r{ r.x * sc, r.y * sc };
            const double2 sum = cadd(u, v);
            x = double2{ sum.x * sc, sum.y * sc };
            y = cmul(csubc(u, v), scaled_r);
        }
        // transform_to_rev's butterfly: (x, y) <- (x + y r, x - y r)  (dwthandler.h:94-191)
        __device__ __forceinline__ void ct_butterfly(double2 &x, double2 &y, double2 r)
        {
            const double2 u = x, v = cmul(y, r);
            x = cadd(u, v);
            y = csubc(u, v);
        }

        // x = sum_j [x_j m (Q/q_j)^-1 mod q_j] (Q/q_j) mod Q as K little-endian words (RNSBase::compose_array, rns.cpp:300-360);
        // m = an optional scalar multiplied into every residue first (1 = none)
        __device__ __forceinline__ void crt_compose(
            uint64_t (&acc)[kMaxComps], const uint64_t *in, uint64_t m, const ModDesc *mods, const uint64_t *punct, const ShoupOp *inv_punct,
            const uint64_t *q_words, unsigned n_log, unsigned K)
        {
            for (unsigned w = 0; w < K; w++)
                acc[w] = 0;
            for (unsigned j = 0; j < K; j++)
            {
                const ShoupOp ip = inv_punct[j];
                uint64_t xj = in[(size_t)j << n_log];
                if (m != 1)
                    xj = mul_mod(xj, barrett64(m, mods[j]), mods[j]);
                const uint64_t y = mul_shoup(xj, ip.w, ip.wq, mods[j].q);

                // acc += y * punct_j  (the product is below Q: K words), then one conditional subtraction of Q
                uint64_t carry = 0;
                for (unsigned w = 0; w < K; w++)
                {
                    uint64_t lo, hi;
                    mul_wide(y, punct[(size_t)j * K + w], lo, hi);
                    const uint64_t s1 = acc[w] + lo;
                    const uint64_t c1 = s1 < lo;
                    const uint64_t s2 = s1 + carry;
                    const uint64_t c2 = s2 < carry;
                    acc[w] = s2;
                    carry = hi + c1 + c2; // hi <= 2^64 - 2, so this does not wrap
                }
                // the sum of two values below Q is below 2Q < 2^(64 K + 1): `carry` is its top bit
                bool ge = carry != 0;
                if (!ge)
                {
                    ge = true;
                    for (int w = (int)K - 1; w >= 0; w--)
                        if (acc[w] != q_words[w])
                        {
                            ge = acc[w] > q_words[w];
                            break;
                        }
                }
                if (ge)
                {
                    uint64_t borrow = 0;
                    for (unsigned w = 0; w < K; w++)
                    {
                        const uint64_t d = acc[w] - q_words[w];
                        const uint64_t b1 = acc[w] < q_words[w];
                        const uint64_t d2 = d - borrow;
                        const uint64_t b2 = d < borrow;
                        acc[w] = d2;
                        borrow = b1 | b2;
                    }
                }
            }
        }

        // decode_internal's composition and scaling of one coefficient (ckks.h:741-781): the centred value times inv_scale, word by
        // word.  `in` = the coefficient's residue under the first prime, the others N words apart.
        __device__ __forceinline__ double compose_scale(const CkksDecodeArgs &a, const uint64_t *in)
        {
            const unsigned K = a.K;
            const double two_pow_64 = 18446744073709551616.0;
            uint64_t acc[kMaxComps];
            crt_compose(acc, in, 1, a.mods, a.punct, a.inv_punct, a.q_words, a.n_log, K);
            bool upper = true; // acc >= upper_half_threshold
            for (int w = (int)K - 1; w >= 0; w--)
                if (acc[w] != a.half_words[w])
                {
                    upper = acc[w] > a.half_words[w];
                    break;
                }
            double res = 0.0;
            double scaled_two_pow_64 = a.inv_scale;
            for (unsigned w = 0; w < K; w++, scaled_two_pow_64 *= two_pow_64)
            {
                if (upper)
                {
                    if (acc[w] > a.q_words[w])
                    {
                        const uint64_t diff = acc[w] - a.q_words[w];
                        res += diff ? (double)diff * scaled_two_pow_64 : 0.0;
                    }
                    else
                    {
                        const uint64_t diff = a.q_words[w] - acc[w];
                        res -= diff ? (double)diff * scaled_two_pow_64 : 0.0;
                    }
                }
                else
                {
                    const uint64_t c = acc[w];
                    res += c ? (double)c * scaled_two_pow_64 : 0.0;
                }
            }
            return res;
        }

        // ---------------------------------------------------------------------------------------------------- encode
        // the value of coefficient position `pos` before the transform: the slot value, its conjugate or zero (encode_internal's
        // placement through matrix_reps_index_map_, ckks.h:512-518); a non-finite input marks the item
        __device__ __forceinline__ double2 encode_load(const CkksEncodeArgs &a, const double *vin, size_t pos, size_t slots, bool &bad)
        {
            const uint32_t s = a.inv_map[pos];
            const bool conj = s >= slots;
            const size_t idx = conj ? s - slots : s;
            double2 v{ 0.0, 0.0 };
            if (idx < a.value_count)
            {
                v = a.is_complex ? double2{ vin[2 * idx], vin[2 * idx + 1] } : double2{ vin[idx], 0.0 };
                bad |= !std::isfinite(v.x) || !std::isfinite(v.y);
                if (conj)
                    v.y = -v.y; // std::conj (of a real value: imaginary part -0.0, as the reference's)
            }
            return v;
        }
        // encode_internal after the transform (ckks.h:520-672) for one coefficient: the size check, the rounding and the RNS
        // decomposition.  The reference picks one width for the whole vector from its largest coefficient; the 64-bit, 128-bit and
        // multi-precision branches all compute round(x) mod q exactly, so the width is picked here per coefficient.
        __device__ __forceinline__ void encode_finish(const CkksEncodeArgs &a, size_t item, size_t pos, double x)
        {
            const double two_pow_64 = 18446744073709551616.0;
            if (!(::fabs(x) <= a.coeff_limit))
                atomicMax(a.fail, ~(2 * (a.item0 + (unsigned)item) + 1));
            double coeffd = ::round(x);
            const bool is_negative = std::signbit(coeffd);
            coeffd = ::fabs(coeffd);
            const unsigned K = a.K;
            uint64_t *o = a.words + ((item * K) << a.n_log) + pos;
            if (coeffd < two_pow_64)
            {
                const uint64_t lo = (uint64_t)coeffd;
                for (unsigned j = 0; j < K; j++)
                {
                    const ModDesc md = a.mods[j];
                    const uint64_t r = barrett64(lo, md);
                    o[(size_t)j << a.n_log] = is_negative ? neg_mod(r, md.q) : r;
                }
            }
            else if (coeffd < two_pow_64 * two_pow_64)
            {
                const uint64_t lo = (uint64_t)::fmod(coeffd, two_pow_64), hi = (uint64_t)(coeffd / two_pow_64);
                for (unsigned j = 0; j < K; j++)
                {
                    const ModDesc md = a.mods[j];
                    const uint64_t r = barrett128(lo, hi, md);
                    o[(size_t)j << a.n_log] = is_negative ? neg_mod(r, md.q) : r;
                }
            }
            else
            {
                // the "slow case" (ckks.h:624-672): the rounded double cut into 64-bit words by repeated fmod / division by 2^64
                // (both exact: the divisor is a power of two), at most K words since the coefficient is below the level's modulus,
                // and the K-word integer reduced modulo every prime (RNSBase::decompose -> modulo_uint): Horner from the top word.
                // A NaN or infinite coefficient (a failed item, whose words are unspecified) stops at K words or none.
                uint64_t words[kMaxComps];
                unsigned nw = 0;
                double c = coeffd;
                while (c >= 1 && nw < K)
                {
                    words[nw++] = (uint64_t)::fmod(c, two_pow_64);
                    c /= two_pow_64;
                }
                for (unsigned j = 0; j < K; j++)
                {
                    const ModDesc md = a.mods[j];
                    uint64_t r = 0;
                    for (unsigned w = nw; w-- > 0;)
                        r = barrett128(words[w], r, md);
                    o[(size_t)j << a.n_log] = is_negative ? neg_mod(r, md.q) : r;
                }
            }
        }
        // Gentleman-Sande stage g (gap 2^g) on the LDS block that starts at global position `base`: group i of the stage (global)
        // uses inv_roots[N - 2 m + 1 + i], m = N / 2^(g+1) groups
        template <bool kScaled>
        __device__ __forceinline__ void gs_lds_stage(double2 *lds, const double2 *inv_roots, size_t n, size_t base, unsigned b, unsigned g, double sc)
        {
            const size_t m = (n >> 1) >> g, root_start = n - 2 * m + 1;
            for (unsigned t = threadIdx.x; t < (1u << (b - 1)); t += blockDim.x)
            {
                const unsigned il = t >> g, j = t & ((1u << g) - 1);
                const unsigned xi = (il << (g + 1)) + j, yi = xi + (1u << g);
                const double2 r = inv_roots[root_start + (base >> (g + 1)) + il];
                double2 x = lds[xi], y = lds[yi];
                if (kScaled)
                    gs_butterfly_scaled(x, y, r, sc);
                else
                    gs_butterfly(x, y, r);
                lds[xi] = x;
                lds[yi] = y;
            }
            __syncthreads();
        }
        // pass 1 of encode (or the whole of it, kWhole): one workgroup = one block of 2^block_log positions of one vector in LDS,
        // stages 0 .. block_log - 1.  grid (N / 2^block_log, items)
        template <bool kWhole>
        __global__ void __launch_bounds__(kBlock) ckks_encode_block_kernel(CkksEncodeArgs a)
        {
            HIP_DYNAMIC_SHARED(double2, lds)
            const unsigned b = a.block_log;
            const size_t n = size_t(1) << a.n_log, slots = n >> 1, item = blockIdx.y, base = (size_t)blockIdx.x << b;
            const double *vin = a.values + item * a.value_count * (a.is_complex ? 2 : 1);
            bool bad = false;
            for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
                lds[p] = encode_load(a, vin, base + p, slots, bad);
            if (bad)
                atomicMax(a.fail, ~(2 * (a.item0 + (unsigned)item)));
            __syncthreads();
            const unsigned plain_stages = kWhole ? b - 1 : b;
            for (unsigned g = 0; g < plain_stages; g++)
                gs_lds_stage<false>(lds, a.inv_roots, n, base, b, g, 0.0);
            if (kWhole)
            {
                gs_lds_stage<true>(lds, a.inv_roots, n, base, b, b - 1, a.fix);
                for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
                    encode_finish(a, item, base + p, lds[p].x);
            }
            else
            {
                double2 *dst = a.mid + (item << a.n_log) + base;
                for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
                    dst[p] = lds[p];
            }
        }
        // pass 2 of encode: one thread = one column {c + k 2^block_log : k < 2^S} in registers, stages block_log .. n_log - 1 (the
        // last one scaled), then the rounding / decomposition of its 2^S coefficients.  grid (2^block_log / blockDim, items)
        template <unsigned S>
        __global__ void __launch_bounds__(kBlock) ckks_encode_column_kernel(CkksEncodeArgs a)
        {
            constexpr unsigned R = 1u << S;
            const unsigned b = a.block_log;
            const size_t n = size_t(1) << a.n_log, item = blockIdx.y, c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
            const double2 *src = a.mid + (item << a.n_log) + c;
            double2 v[R];
#pragma unroll
            for (unsigned k = 0; k < R; k++)
                v[k] = src[(size_t)k << b];
#pragma unroll
            for (unsigned s = 0; s < S; s++)
            {
                // stage g = b + s pairs k and k + 2^s; its group is k >> (s + 1), the same for every column
                const size_t m = (n >> 1) >> (b + s), root_start = n - 2 * m + 1;
#pragma unroll
                for (unsigned k = 0; k < R; k++)
                    if (!((k >> s) & 1))
                    {
                        const double2 r = a.inv_roots[root_start + (k >> (s + 1))];
                        if (s + 1 == S)
                            gs_butterfly_scaled(v[k], v[k | (1u << s)], r, a.fix);
                        else
                            gs_butterfly(v[k], v[k | (1u << s)], r);
                    }
            }
#pragma unroll
            for (unsigned k = 0; k < R; k++)
                encode_finish(a, item, c + ((size_t)k << b), v[k].x);
        }

        // ---------------------------------------------------------------------------------------------------- decode
        // pass 1 of decode: one workgroup = C = 256 / 2^S columns {c + k 2^block_log : k < 2^S}, one thread per coefficient
        // composed and scaled on load (the K^2 word products are the bulk of decode), then Cooley-Tukey stages n_log - 1 ..
        // block_log on the columns in LDS (group i of stage g uses roots[m + i], m = N / 2^(g+1); the group depends on k only)
        template <unsigned S>
        __global__ void __launch_bounds__(kBlock) ckks_decode_column_kernel(CkksDecodeArgs a)
        {
            __shared__ double2 lds[kBlock];
            const unsigned b = a.block_log, C = blockDim.x >> S;
            const size_t n = size_t(1) << a.n_log, item = blockIdx.y;
            const unsigned col = threadIdx.x % C, k = threadIdx.x / C;
            const size_t c = (size_t)blockIdx.x * C + col, pos = c + ((size_t)k << b);
            lds[threadIdx.x] = double2{ compose_scale(a, a.residues + ((item * a.K) << a.n_log) + pos), 0.0 };
            __syncthreads();
            for (int s = (int)S - 1; s >= 0; s--)
            {
                const size_t m = (n >> 1) >> (b + s);
                if (threadIdx.x < (blockDim.x >> 1))
                {
                    const unsigned pc = threadIdx.x % C, j = threadIdx.x / C;
                    const unsigned kx = ((j >> s) << (s + 1)) | (j & ((1u << s) - 1));
                    double2 x = lds[kx * C + pc], y = lds[(kx | (1u << s)) * C + pc];
                    ct_butterfly(x, y, a.roots[m + (kx >> (s + 1))]);
                    lds[kx * C + pc] = x;
                    lds[(kx | (1u << s)) * C + pc] = y;
                }
                __syncthreads();
            }
            a.mid[(item << a.n_log) + pos] = lds[threadIdx.x];
        }
        // pass 2 of decode (or the whole of it, kWhole: composed and scaled on load): one block of 2^block_log positions in LDS,
        // stages block_log - 1 .. 0, stored through the index map straight into the slots (decode_internal's last loop)
        template <bool kWhole>
        __global__ void __launch_bounds__(kBlock) ckks_decode_block_kernel(CkksDecodeArgs a)
        {
            HIP_DYNAMIC_SHARED(double2, lds)
            const unsigned b = a.block_log;
            const size_t n = size_t(1) << a.n_log, slots = n >> 1, item = blockIdx.y, base = (size_t)blockIdx.x << b;
            if (kWhole)
            {
                const uint64_t *in = a.residues + ((item * a.K) << a.n_log) + base;
                for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
                    lds[p] = double2{ compose_scale(a, in + p), 0.0 };
            }
            else
            {
                const double2 *src = a.mid + (item << a.n_log) + base;
                for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
                    lds[p] = src[p];
            }
            __syncthreads();
            for (int g = (int)b - 1; g >= 0; g--)
            {
                const size_t m = (n >> 1) >> g;
                for (unsigned t = threadIdx.x; t < (1u << (b - 1)); t += blockDim.x)
                {
                    const unsigned il = t >> g, j = t & ((1u << g) - 1);
                    const unsigned xi = (il << (g + 1)) + j, yi = xi + (1u << g);
                    double2 x = lds[xi], y = lds[yi];
                    ct_butterfly(x, y, a.roots[m + (base >> (g + 1)) + il]);
                    lds[xi] = x;
                    lds[yi] = y;
                }
                __syncthreads();
            }
            for (unsigned p = threadIdx.x; p < (1u << b); p += blockDim.x)
            {
                const uint32_t s = a.inv_map[base + p];
                if (s >= slots)
                    continue;
                const double2 v = lds[p];
                if (a.want_complex)
                {
                    a.out[2 * (item * slots + s)] = v.x;
                    a.out[2 * (item * slots + s) + 1] = v.y;
                }
                else
                    a.out[item * slots + s] = v.x; // from_complex<double>: the real part
            }
        }
        // significant bits of the centred CRT value of every coefficient, maximum per vector (poly_infty_norm_coeffmod)
        __global__ void __launch_bounds__(kBlock) crt_norm_bits_kernel(
            const ModDesc *mods, const uint64_t *residues, const uint64_t *punct, const ShoupOp *inv_punct, const uint64_t *q_words,
            const uint64_t *half_words, uint64_t m, unsigned *out_bits, unsigned n_log, unsigned K, size_t count)
        {
            const size_t nmask = (size_t(1) << n_log) - 1;
            for (size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x; t < count; t += (size_t)gridDim.x * kBlock)
            {
                const size_t vec = t >> n_log, i = t & nmask;
                uint64_t acc[kMaxComps];
                crt_compose(acc, residues + ((vec * K) << n_log) + i, m, mods, punct, inv_punct, q_words, n_log, K);
                bool upper = true; // acc >= (Q + 1) / 2: the representative is Q - acc
                for (int w = (int)K - 1; w >= 0; w--)
                    if (acc[w] != half_words[w])
                    {
                        upper = acc[w] > half_words[w];
                        break;
                    }
                if (upper)
                {
                    uint64_t borrow = 0;
                    for (unsigned w = 0; w < K; w++)
                    {
                        const uint64_t d = q_words[w] - acc[w];
                        const uint64_t b1 = q_words[w] < acc[w];
                        const uint64_t d2 = d - borrow;
                        const uint64_t b2 = d < borrow;
                        acc[w] = d2;
                        borrow = b1 | b2;
                    }
                }
                unsigned bits = 0;
                for (int w = (int)K - 1; w >= 0; w--)
                    if (acc[w])
                    {
                        bits = (unsigned)w * 64 + (64 - __builtin_clzll(acc[w]));
                        break;
                    }
                atomicMax(out_bits + vec, bits);
            }
        }
    } // namespace

    hipError_t k_ckks_encode(const CkksEncodeArgs &a, unsigned items, hipStream_t s)
    {
        const unsigned b = a.block_log, S = a.n_log - b;
        if (!items)
            return hipSuccess;
        if (b < 1 || b > kFftLdsLog || S > kFftMaxColumnLog)
            return hipErrorInvalidValue;
        const dim3 bgrid(1u << S, items), bthreads(std::min(kBlock, 1u << (b - 1)));
        const size_t lds = sizeof(double2) << b;
        if (!S)
        {
            hipLaunchKernelGGL(ckks_encode_block_kernel<true>, bgrid, bthreads, lds, s, a);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(ckks_encode_block_kernel<false>, bgrid, bthreads, lds, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        const unsigned cthreads = std::min(kBlock, 1u << b);
        const dim3 cgrid((1u << b) / cthreads, items);
        switch (S)
        {
        case 1: hipLaunchKernelGGL(ckks_encode_column_kernel<1>, cgrid, dim3(cthreads), 0, s, a); break;
        case 2: hipLaunchKernelGGL(ckks_encode_column_kernel<2>, cgrid, dim3(cthreads), 0, s, a); break;
        case 3: hipLaunchKernelGGL(ckks_encode_column_kernel<3>, cgrid, dim3(cthreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL(ckks_encode_column_kernel<4>, cgrid, dim3(cthreads), 0, s, a); break;
        default: hipLaunchKernelGGL(ckks_encode_column_kernel<5>, cgrid, dim3(cthreads), 0, s, a); break;
        }
        return hipGetLastError();
    }
    hipError_t k_ckks_decode(const CkksDecodeArgs &a, unsigned items, hipStream_t s)
    {
        const unsigned b = a.block_log, S = a.n_log - b;
        if (!items)
            return hipSuccess;
        if (b < 1 || b > kFftLdsLog || S > kFftMaxColumnLog)
            return hipErrorInvalidValue;
        const dim3 bgrid(1u << S, items), bthreads(std::min(kBlock, 1u << (b - 1)));
        const size_t lds = sizeof(double2) << b;
        if (!S)
        {
            hipLaunchKernelGGL(ckks_decode_block_kernel<true>, bgrid, bthreads, lds, s, a);
            return hipGetLastError();
        }
        // C = 256 / 2^S columns per workgroup (at least 8: S <= 5), fewer when the block has fewer columns
        const unsigned ccols = std::min(kBlock >> S, 1u << b);
        const unsigned cthreads = ccols << S;
        const dim3 cgrid((1u << b) / ccols, items);
        switch (S)
        {
        case 1: hipLaunchKernelGGL(ckks_decode_column_kernel<1>, cgrid, dim3(cthreads), 0, s, a); break;
        case 2: hipLaunchKernelGGL(ckks_decode_column_kernel<2>, cgrid, dim3(cthreads), 0, s, a); break;
        case 3: hipLaunchKernelGGL(ckks_decode_column_kernel<3>, cgrid, dim3(cthreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL(ckks_decode_column_kernel<4>, cgrid, dim3(cthreads), 0, s, a); break;
        default: hipLaunchKernelGGL(ckks_decode_column_kernel<5>, cgrid, dim3(cthreads), 0, s, a); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        hipLaunchKernelGGL(ckks_decode_block_kernel<false>, bgrid, bthreads, lds, s, a);
        return hipGetLastError();
    }
    hipError_t k_crt_norm_bits(const ModDesc *mods, const uint64_t *residues, const uint64_t *punct, const ShoupOp *inv_punct,
                               const uint64_t *q_words, const uint64_t *half_words, uint64_t m, unsigned *out_bits, unsigned n_log, unsigned K,
                               unsigned batch, hipStream_t s)
    {
        const size_t count = (size_t)batch << n_log;
        hipLaunchKernelGGL(crt_norm_bits_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, mods, residues, punct, inv_punct, q_words, half_words,
                           m, out_bits, n_log, K, count);
        return hipGetLastError();
    }
} // namespace sealhip
