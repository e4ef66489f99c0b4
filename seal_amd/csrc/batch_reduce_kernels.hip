// See batch_reduce_kernels.h.  One thread = two adjacent words of one output row (N is even, rows are 16-byte aligned); the grid is
// flat in x (one thread per output pair) and, when the group is cut, the slices sit in y.
#include "batch_reduce_kernels.h"
#include "stream_device.h"
#include <algorithm>

namespace sealhip
{
    namespace
    {
        constexpr unsigned kBlock = 256;

        // ---- lazy accumulation.  Every prime is below 2^60 (a coefficient modulus has at most 60 bits; include/sealhip.h section 1b
        // relies on the same bound), so a canonical word is at most 2^60 - 1.
        //   sums:     T words add up to at most T (2^60 - 1) < 2^64  as long as  T <= 2^(64 - 60) = 16
        //   products: a product of two canonical words is at most (2^60 - 1)^2 < 2^120, so T of them add up to less than 2^128
        //             as long as  T <= 2^(128 - 120) = 256
        // A run of at most that many terms is added as a plain 64-bit / 128-bit integer, reduced once (barrett64 / barrett128, whose
        // only requirements are a value below 2^64 / 2^128 and q < 2^62) and added to the running canonical total with add_mod.
        constexpr unsigned kPrimeBits = 60;
        constexpr unsigned kSumFlush = 1u << (64 - kPrimeBits);
        constexpr unsigned kDotFlush = 1u << (128 - 2 * kPrimeBits);
        static_assert(kSumFlush == 16 && (unsigned __int128)kSumFlush * ((uint64_t(1) << kPrimeBits) - 1) <= ~uint64_t(0),
                      "kSumFlush words below 2^60 must fit 64 bits");
        static_assert(kDotFlush == 256 && (unsigned __int128)((uint64_t(1) << kPrimeBits) - 1) * ((uint64_t(1) << kPrimeBits) - 1) <=
                                              ~(unsigned __int128)0 / kDotFlush,
                      "kDotFlush products of words below 2^60 must fit 128 bits");
        // the ciphertext x ciphertext product's middle polynomial takes TWO products per item (x0 y1 + x1 y0), so a run of it is half
        // as many items; the outer two sums are flushed at the same interval
        constexpr unsigned kDotItemsFlush = kDotFlush / 2;
        static_assert(kDotItemsFlush == 128 && 2 * kDotItemsFlush <= kDotFlush, "two products per item: kDotFlush of them in kDotItemsFlush items");

        // ---- the cut of a small result (tuning values; tools/batch_reduce_rate.py sweeps them, DESIGN.md has the table)
        constexpr size_t kSliceBelowThreads = size_t(1) << 17; // launches of fewer threads than this are cut
        constexpr size_t kSliceTargetThreads = size_t(1) << 19; // ... into as many slices as bring them to about this many
        constexpr size_t kSliceMinTerms = 4;                    // but a slice adds at least this many items
        constexpr unsigned kMaxSlices = 64;

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

        // strides in words
        struct SumGeom
        {
            size_t src_plane, src_item, src_term; // source word of (plane p, output item o, term t): p * src_plane + o * src_item + t * src_term
            size_t dst_plane, dst_slice;          // result word of (slice s, plane p): s * dst_slice + p * dst_plane
            size_t pairs;                         // size * out_items * K * N / 2
            unsigned out_items, terms, per_slice; // slice s adds the terms [s * per_slice, min(terms, (s + 1) * per_slice))
            unsigned n_log, K;
        };

        // OPERANDS: the source is a ciphertext (read once: non-temporal) and not the scratch of the slices; FINAL: the result is the
        // ciphertext (written once: non-temporal) and not scratch that the next launch reads
        template <bool OPERANDS, bool FINAL>
        __global__ void __launch_bounds__(kBlock) sum_items_kernel(const ModDesc *mods, const uint64_t *src, uint64_t *dst, SumGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.pairs)
                return;
            const size_t i = 2 * w, j = i & ((size_t(1) << g.n_log) - 1);
            const unsigned row = (unsigned)(i >> g.n_log); // (p * out_items + o) * K + k
            const unsigned k = row % g.K, po = row / g.K, o = po % g.out_items, p = po / g.out_items;
            const ModDesc md = mods[k];
            const unsigned t0 = blockIdx.y * g.per_slice, t1 = g.terms - t0 < g.per_slice ? g.terms : t0 + g.per_slice;
            const size_t inner = ((size_t)k << g.n_log) + j;
            const uint64_t *s = src + p * g.src_plane + o * g.src_item + t0 * g.src_term + inner;
            uint64_t tot0 = 0, tot1 = 0;
            for (unsigned t = t0; t < t1;)
            {
                const unsigned end = t1 - t < kSumFlush ? t1 : t + kSumFlush;
                uint64_t acc0 = 0, acc1 = 0;
#pragma unroll 4
                for (; t < end; t++, s += g.src_term)
                {
                    uint64_t a0, a1;
                    ld2<OPERANDS>(s, a0, a1);
                    acc0 += a0;
                    acc1 += a1;
                }
                tot0 = add_mod(tot0, barrett64(acc0, md), md.q);
                tot1 = add_mod(tot1, barrett64(acc1, md), md.q);
            }
            uint64_t *d = dst + blockIdx.y * g.dst_slice + p * g.dst_plane + (((size_t)o * g.K) << g.n_log) + inner;
            if (FINAL)
                st2_nt(d, tot0, tot1);
            else
                st2(d, tot0, tot1);
        }

        struct DotGeom
        {
            size_t a_plane;              // words between two planes of the operand
            size_t dst_plane, dst_slice; // as SumGeom
            size_t pairs;                // out_items * K * N / 2
            size_t words;                // K * N: one item of one plane
            unsigned group, per_slice;   // slice s adds the items [s * per_slice, min(group, (s + 1) * per_slice)) of every group
            unsigned n_log, K;
        };
        struct U128
        {
            uint64_t lo, hi;
        };
        __device__ __forceinline__ void mac128(U128 &acc, uint64_t a, uint64_t b)
        {
            uint64_t lo, hi;
            mul_wide(a, b, lo, hi);
            acc.lo += lo;
            acc.hi += hi + (acc.lo < lo);
        }

        // SIZE planes of the operand per thread, over which it keeps each plaintext pair in registers
        template <unsigned SIZE, bool FINAL>
        __global__ void __launch_bounds__(kBlock) dot_plain_items_kernel(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, uint64_t *dst,
                                                                         DotGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.pairs)
                return;
            const size_t i = 2 * w, j = i & ((size_t(1) << g.n_log) - 1);
            const unsigned row = (unsigned)(i >> g.n_log); // o * K + k
            const unsigned k = row % g.K, o = row / g.K;
            const ModDesc md = mods[k];
            const unsigned t0 = blockIdx.y * g.per_slice, t1 = g.group - t0 < g.per_slice ? g.group : t0 + g.per_slice;
            const size_t inner = ((size_t)k << g.n_log) + j;
            const size_t first = ((size_t)o * g.group + t0) * g.words + inner; // item o * group + t0, component k, coefficient j
            const uint64_t *ap = a + first, *pp = pl + first;
            uint64_t tot[SIZE][2];
            for (unsigned p = 0; p < SIZE; p++)
                tot[p][0] = tot[p][1] = 0;
            for (unsigned t = t0; t < t1;)
            {
                const unsigned end = t1 - t < kDotFlush ? t1 : t + kDotFlush;
                U128 acc[SIZE][2];
                for (unsigned p = 0; p < SIZE; p++)
                    acc[p][0] = acc[p][1] = U128{ 0, 0 };
#pragma unroll 2
                for (; t < end; t++, ap += g.words, pp += g.words)
                {
                    uint64_t p0, p1;
                    ld2<true>(pp, p0, p1);
                    for (unsigned p = 0; p < SIZE; p++)
                    {
                        uint64_t a0, a1;
                        ld2<true>(ap + p * g.a_plane, a0, a1);
                        mac128(acc[p][0], a0, p0);
                        mac128(acc[p][1], a1, p1);
                    }
                }
                for (unsigned p = 0; p < SIZE; p++)
                {
                    tot[p][0] = add_mod(tot[p][0], barrett128(acc[p][0].lo, acc[p][0].hi, md), md.q);
                    tot[p][1] = add_mod(tot[p][1], barrett128(acc[p][1].lo, acc[p][1].hi, md), md.q);
                }
            }
            uint64_t *d = dst + blockIdx.y * g.dst_slice + (((size_t)o * g.K) << g.n_log) + inner;
            for (unsigned p = 0; p < SIZE; p++)
            {
                if (FINAL)
                    st2_nt(d + p * g.dst_plane, tot[p][0], tot[p][1]);
                else
                    st2(d + p * g.dst_plane, tot[p][0], tot[p][1]);
            }
        }

        // ---- ciphertext x ciphertext: r[.][o] = sum_i x[.][o g + i] (x) y[.][o g + i], the size-2 x size-2 tensor product
        struct DotItemsGeom
        {
            size_t x_plane, y_plane;     // words between the two planes of each operand
            size_t dst_plane, dst_slice; // as SumGeom
            size_t pairs;                // out_items * K * N / 2
            size_t words;                // K * N: one item of one plane
            unsigned group, per_slice;   // slice s adds the items [s * per_slice, min(group, (s + 1) * per_slice)) of every group
            unsigned n_log, K;
        };
        __device__ __forceinline__ void add128(U128 &acc, uint64_t lo, uint64_t hi)
        {
            acc.lo += lo;
            acc.hi += hi + (acc.lo < lo);
        }

        // c0 += x0 y0, c1 += x0 y1 + x1 y0, c2 += x1 y1 per item, as plain 128-bit integers for kDotItemsFlush items at a time.
        // SQUARE: y is x - two loads per item, and the middle sum takes the one product x0 x1 twice (the same integer as x0 y1 + x1 y0)
        template <bool SQUARE, bool FINAL>
        __global__ void __launch_bounds__(kBlock) dot_items_kernel(const ModDesc *mods, const uint64_t *x, const uint64_t *y, uint64_t *dst,
                                                                   DotItemsGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.pairs)
                return;
            const size_t i = 2 * w, j = i & ((size_t(1) << g.n_log) - 1);
            const unsigned row = (unsigned)(i >> g.n_log); // o * K + k
            const unsigned k = row % g.K, o = row / g.K;
            const ModDesc md = mods[k];
            const unsigned t0 = blockIdx.y * g.per_slice, t1 = g.group - t0 < g.per_slice ? g.group : t0 + g.per_slice;
            const size_t inner = ((size_t)k << g.n_log) + j;
            const size_t first = ((size_t)o * g.group + t0) * g.words + inner; // item o * group + t0, component k, coefficient j
            const uint64_t *xp = x + first, *yp = y + first;
            uint64_t tot[3][2];
            for (unsigned p = 0; p < 3; p++)
                tot[p][0] = tot[p][1] = 0;
            for (unsigned t = t0; t < t1;)
            {
                const unsigned end = t1 - t < kDotItemsFlush ? t1 : t + kDotItemsFlush;
                U128 acc[3][2];
                for (unsigned p = 0; p < 3; p++)
                    acc[p][0] = acc[p][1] = U128{ 0, 0 };
#pragma unroll 2
                for (; t < end; t++, xp += g.words, yp += g.words)
                {
                    uint64_t x0[2], x1[2];
                    ld2<true>(xp, x0[0], x0[1]);
                    ld2<true>(xp + g.x_plane, x1[0], x1[1]);
                    if (SQUARE)
                    {
                        for (unsigned l = 0; l < 2; l++)
                        {
                            uint64_t lo, hi;
                            mul_wide(x0[l], x1[l], lo, hi);
                            mac128(acc[0][l], x0[l], x0[l]);
                            add128(acc[1][l], lo, hi);
                            add128(acc[1][l], lo, hi);
                            mac128(acc[2][l], x1[l], x1[l]);
                        }
                    }
                    else
                    {
                        uint64_t y0[2], y1[2];
                        ld2<true>(yp, y0[0], y0[1]);
                        ld2<true>(yp + g.y_plane, y1[0], y1[1]);
                        for (unsigned l = 0; l < 2; l++)
                        {
                            mac128(acc[0][l], x0[l], y0[l]);
                            mac128(acc[1][l], x0[l], y1[l]);
                            mac128(acc[1][l], x1[l], y0[l]);
                            mac128(acc[2][l], x1[l], y1[l]);
                        }
                    }
                }
                for (unsigned p = 0; p < 3; p++)
                {
                    tot[p][0] = add_mod(tot[p][0], barrett128(acc[p][0].lo, acc[p][0].hi, md), md.q);
                    tot[p][1] = add_mod(tot[p][1], barrett128(acc[p][1].lo, acc[p][1].hi, md), md.q);
                }
            }
            uint64_t *d = dst + blockIdx.y * g.dst_slice + (((size_t)o * g.K) << g.n_log) + inner;
            for (unsigned p = 0; p < 3; p++)
            {
                if (FINAL)
                    st2_nt(d + p * g.dst_plane, tot[p][0], tot[p][1]);
                else
                    st2(d + p * g.dst_plane, tot[p][0], tot[p][1]);
            }
        }

        // one thread per pair, rows numbered in 32 bits: false when the launch would not fit
        inline bool flat_grid(size_t pairs, unsigned n_log, unsigned &blocks)
        {
            const size_t b = (pairs + kBlock - 1) / kBlock;
            blocks = (unsigned)b;
            return b <= 0x7fffffffu && ((2 * pairs) >> n_log) <= 0xffffffffu;
        }
        // the cut: per_slice items per slice and the slices that leaves non-empty; false = the arguments do not describe one
        inline bool cut(size_t group, unsigned &slices, unsigned &per_slice)
        {
            if (!slices || slices > kMaxSlices || slices > group || group > 0xffffffffu)
                return false;
            per_slice = (unsigned)((group + slices - 1) / slices);
            slices = (unsigned)((group + per_slice - 1) / per_slice);
            return true;
        }

        template <bool OPERANDS, bool FINAL>
        hipError_t launch_sum(const ModDesc *mods, const uint64_t *src, uint64_t *dst, const SumGeom &g, unsigned slices, hipStream_t s)
        {
            unsigned blocks;
            if (!flat_grid(g.pairs, g.n_log, blocks))
                return hipErrorInvalidValue;
            hipLaunchKernelGGL((sum_items_kernel<OPERANDS, FINAL>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, src, dst, g);
            return hipGetLastError();
        }
        // adds the slices in scratch [slices][size][out_items][K][N] into the result
        hipError_t combine_slices(const ModDesc *mods, const uint64_t *scratch, uint64_t *r, size_t r_stride, unsigned size, unsigned n_log,
                                  unsigned K, size_t out_items, unsigned slices, hipStream_t s)
        {
            const size_t words = (size_t)K << n_log, out_plane = out_items * words;
            const SumGeom g{ out_plane, words, size * out_plane, r_stride, 0, size * out_plane / 2, (unsigned)out_items, slices, slices, n_log, K };
            return launch_sum<false, true>(mods, scratch, r, g, 1, s);
        }

        template <unsigned SIZE>
        hipError_t launch_dot(const ModDesc *mods, const uint64_t *a, const uint64_t *pl, uint64_t *dst, const DotGeom &g, unsigned slices,
                              bool final, hipStream_t s)
        {
            unsigned blocks;
            if (!flat_grid(g.pairs, g.n_log, blocks))
                return hipErrorInvalidValue;
            if (final)
                hipLaunchKernelGGL((dot_plain_items_kernel<SIZE, true>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, a, pl, dst, g);
            else
                hipLaunchKernelGGL((dot_plain_items_kernel<SIZE, false>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, a, pl, dst, g);
            return hipGetLastError();
        }
        template <bool SQUARE>
        hipError_t launch_dot_items(const ModDesc *mods, const uint64_t *x, const uint64_t *y, uint64_t *dst, const DotItemsGeom &g,
                                    unsigned slices, bool final, hipStream_t s)
        {
            unsigned blocks;
            if (!flat_grid(g.pairs, g.n_log, blocks))
                return hipErrorInvalidValue;
            if (final)
                hipLaunchKernelGGL((dot_items_kernel<SQUARE, true>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, x, y, dst, g);
            else
                hipLaunchKernelGGL((dot_items_kernel<SQUARE, false>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, x, y, dst, g);
            return hipGetLastError();
        }
    } // namespace

    unsigned batch_reduce_sum_flush()
    {
        return kSumFlush;
    }
    unsigned batch_reduce_dot_flush()
    {
        return kDotFlush;
    }
    unsigned batch_reduce_dot_items_flush()
    {
        return kDotItemsFlush;
    }
    unsigned batch_reduce_slices(size_t threads, size_t group)
    {
        if (!threads || threads >= kSliceBelowThreads || group < 2 * kSliceMinTerms)
            return 1;
        const size_t want = (kSliceTargetThreads + threads - 1) / threads;
        unsigned slices = (unsigned)std::min<size_t>(std::min<size_t>(want, group / kSliceMinTerms), kMaxSlices), per_slice;
        cut(group, slices, per_slice);
        return slices;
    }

    hipError_t k_sum_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, uint64_t *r, size_t r_stride, unsigned size, unsigned n_log,
                           unsigned K, size_t out_items, size_t group, unsigned slices, uint64_t *scratch, hipStream_t s)
    {
        const size_t words = (size_t)K << n_log, out_plane = out_items * words;
        if (!size || !out_plane || !group)
            return hipSuccess;
        unsigned per_slice;
        if (!cut(group, slices, per_slice) || out_items > 0xffffffffu || (slices > 1 && !scratch))
            return hipErrorInvalidValue;
        SumGeom g{ a_stride, group * words, words, r_stride, 0, size * out_plane / 2, (unsigned)out_items, (unsigned)group, per_slice, n_log, K };
        if (slices == 1)
            return launch_sum<true, true>(mods, a, r, g, 1, s);
        g.dst_plane = out_plane;
        g.dst_slice = size * out_plane;
        hipError_t e = launch_sum<true, false>(mods, a, scratch, g, slices, s);
        if (e != hipSuccess)
            return e;
        return combine_slices(mods, scratch, r, r_stride, size, n_log, K, out_items, slices, s);
    }

    hipError_t k_dot_plain_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride,
                                 unsigned size, unsigned n_log, unsigned K, size_t out_items, size_t group, unsigned slices, uint64_t *scratch,
                                 hipStream_t s)
    {
        const size_t words = (size_t)K << n_log, out_plane = out_items * words;
        if (!size || !out_plane || !group)
            return hipSuccess;
        unsigned per_slice;
        if (!cut(group, slices, per_slice) || out_items > 0xffffffffu || (slices > 1 && !scratch))
            return hipErrorInvalidValue;
        const bool final = slices == 1;
        uint64_t *dst = final ? r : scratch;
        DotGeom g{ a_stride, final ? r_stride : out_plane, final ? 0 : size * out_plane, out_plane / 2, words, (unsigned)group, per_slice, n_log, K };
        // three planes at a time, then two or one: the plaintexts are read once for size <= 3
        for (unsigned p = 0; p < size;)
        {
            const unsigned take = std::min(3u, size - p);
            const uint64_t *ap = a + p * a_stride;
            uint64_t *dp = dst + p * g.dst_plane;
            hipError_t e = take == 3   ? launch_dot<3>(mods, ap, pl, dp, g, slices, final, s)
                           : take == 2 ? launch_dot<2>(mods, ap, pl, dp, g, slices, final, s)
                                       : launch_dot<1>(mods, ap, pl, dp, g, slices, final, s);
            if (e != hipSuccess)
                return e;
            p += take;
        }
        if (final)
            return hipSuccess;
        return combine_slices(mods, scratch, r, r_stride, size, n_log, K, out_items, slices, s);
    }

    hipError_t k_dot_items(const ModDesc *mods, const uint64_t *x, size_t x_stride, const uint64_t *y, size_t y_stride, uint64_t *r,
                           size_t r_stride, unsigned n_log, unsigned K, size_t out_items, size_t group, unsigned slices, uint64_t *scratch,
                           hipStream_t s)
    {
        const size_t words = (size_t)K << n_log, out_plane = out_items * words;
        if (!out_plane || !group)
            return hipSuccess;
        unsigned per_slice;
        if (!cut(group, slices, per_slice) || out_items > 0xffffffffu || (slices > 1 && !scratch))
            return hipErrorInvalidValue;
        const bool final = slices == 1, square = x == y && x_stride == y_stride;
        uint64_t *dst = final ? r : scratch;
        const DotItemsGeom g{ x_stride, y_stride, final ? r_stride : out_plane, final ? 0 : 3 * out_plane, out_plane / 2, words, (unsigned)group,
                              per_slice, n_log, K };
        hipError_t e = square ? launch_dot_items<true>(mods, x, y, dst, g, slices, final, s)
                              : launch_dot_items<false>(mods, x, y, dst, g, slices, final, s);
        if (e != hipSuccess || final)
            return e;
        return combine_slices(mods, scratch, r, r_stride, 3, n_log, K, out_items, slices, s);
    }
} // namespace sealhip
