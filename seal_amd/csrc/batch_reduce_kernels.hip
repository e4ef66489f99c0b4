// See batch_reduce_kernels.h.  Two skeletons, each with one launch path and one host path:
// - reduce_items_kernel, one output item per thread: one thread = two adjacent words of one output row (N is even, rows are 16-byte
//   aligned); the grid is flat in x (one thread per output pair).  What a reduction adds per term is its Term (SumTerm,
//   DotPlainTerm, DotItemsTerm, DotScalarsTerm), which items its terms are is its Walk (ConsecutiveWalk, MappedWalk); launch_reduce
//   and reduce_items are the launch and the host path.
// - the tiled products (the matrix products and the scalar weights), a TILE of output items per thread, so that each loaded operand
//   word is used for all of them: one geometry (TileGeom), one prologue (TileThread), two bodies - matmul_words_kernel with its term
//   (MatmulItemsTerm, MatmulPlainTerm) and matmul_scalars_kernel, whose weights are scalar loads -, launch_tiled and tiled_reduce;
//   conv2d_scalars_kernel is the second body with another walk: its operand is found in an image, not in a dense matrix.
// Both share the accumulators and flush intervals, the accesses, the flat grid with the slices of a cut in y, the cut and the sum of
// the slices.
#include "batch_reduce_kernels.h"
#include "stream_device.h"
#include <algorithm>
#include <type_traits>

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

        // strides in words.  A row of the grid is (p * out_items + o) * K + k: `pairs` counts the planes p the grid holds (all of them
        // for the sum, one for the products, whose threads loop over their planes)
        struct ReduceGeom
        {
            size_t a_plane, b_plane;              // words between two planes of the first / second operand
            size_t item, term;                    // operand word of (output item o, term t): o * item + t * term
            size_t dst_plane, dst_slice;          // result word of (slice s, plane p): s * dst_slice + p * dst_plane
            size_t pairs;                         // grid planes * out_items * K * N / 2
            unsigned out_items, terms, per_slice; // slice s adds the terms [s * per_slice, min(terms, (s + 1) * per_slice))
            unsigned n_log, K;
        };

        // ---- the walks: which operand items the terms of output item o are.  A Walk gives the slice's range of terms [t0, t1) of
        // a row and moves the operand pointers from term to term; the kernel does not know which one it runs with.
        // Consecutive groups: term t of output item o is item o * group + t of both operands (the strides are ReduceGeom's item, term)
        struct ConsecutiveWalk
        {
            static constexpr bool kMapped = false;
        };
        // An item map (batch_reduce_kernels.h: ItemWalk): row o has the terms off[o] .. off[o + 1] - 1 of two lists of item numbers,
        // 32-bit words in HBM; term t is item first[t] of the first operand and second[t] of the second.  Here ReduceGeom's term is
        // the words of one item ([K][N], below 2^32) and item, terms are not used: an operand address costs one 32 x 32 -> 64
        // multiply-add per term.  per_slice is sized from the longest row; a slice past the end of a short row adds nothing and
        // stores zeros.
        // UNIFORM: a wave covers 128 consecutive words and rows are N words, so from N = 128 on a wave never leaves its row - the row
        // number is moved to an SGPR and offsets and item numbers are read through the constant address space (scalar loads, one per
        // wave and term, uniform trip counts).  Below that the lanes of a wave sit in rows of different length: per-lane loads,
        // divergent trip counts and flushes.
        template <bool UNIFORM>
        struct MappedWalk
        {
            static constexpr bool kMapped = true, kUniform = UNIFORM;
            const uint32_t *off, *first, *second;
            static __device__ __forceinline__ unsigned ld(const uint32_t *p, unsigned i)
            {
                if (UNIFORM)
                    return SHL_UCONST32(p)[i];
                return p[i];
            }
        };

        // ---- the terms.  A Term has kOut result planes per thread, kFlush terms between two reductions of its accumulators (Acc,
        // reduce), the unroll factor of its loop, the waves per SIMD it is built for (the register allocator is held to them:
        // profiles/batch_reduce_unified.txt) and add(): load term t of one output pair and add it to acc[plane][word of the pair].
        // Where a term's second operand is, is the term's business: Second is its word type, second_base() the thread's pointer into
        // item 0 of it (`at`: the thread's words from the start of plane 0 of the first item) and second_at() the pointer of a named
        // item from there - the kernel only hands the walk's item number over
        struct U128
        {
            uint64_t lo, hi;
        };
        __device__ __forceinline__ void add128(U128 &acc, uint64_t lo, uint64_t hi)
        {
            acc.lo += lo;
            acc.hi += hi + (acc.lo < lo);
        }
        __device__ __forceinline__ void mac128(U128 &acc, uint64_t a, uint64_t b)
        {
            uint64_t lo, hi;
            mul_wide(a, b, lo, hi);
            add128(acc, lo, hi);
        }
        // the second operand is items of [K][N] words like the first: plane p, the same words of the item
        struct WordOperand
        {
            using Second = uint64_t;
            static __device__ __forceinline__ const uint64_t *second_base(const uint64_t *b, unsigned p, unsigned, size_t at, const ReduceGeom &g)
            {
                return b + p * g.b_plane + at;
            }
            static __device__ __forceinline__ const uint64_t *second_at(const uint64_t *bp, unsigned item, const ReduceGeom &g)
            {
                return bp + (size_t)item * (unsigned)g.term; // the words of one item, below 2^32
            }
        };
        struct Products : WordOperand // of operands, as 128-bit integers
        {
            using Acc = U128;
            static constexpr bool kOperands = true;
            static constexpr unsigned kUnroll = 2;
            static __device__ __forceinline__ uint64_t reduce(const U128 &acc, const ModDesc &md)
            {
                return barrett128(acc.lo, acc.hi, md);
            }
        };

        // r[p][o] = sum_t a[p][o][t].  OPERANDS: the source is a ciphertext (read once: non-temporal) and not the scratch of the slices
        template <bool OPERANDS>
        struct SumTerm : WordOperand
        {
            using Acc = uint64_t;
            static constexpr bool kOperands = OPERANDS;
            static constexpr unsigned kOut = 1, kFlush = kSumFlush, kUnroll = 4, kWaves = 8;
            static __device__ __forceinline__ uint64_t reduce(uint64_t acc, const ModDesc &md)
            {
                return barrett64(acc, md);
            }
            static __device__ __forceinline__ void add(Acc (&acc)[kOut][2], const uint64_t *a, const uint64_t *, const ReduceGeom &)
            {
                uint64_t a0, a1;
                ld2<OPERANDS>(a, a0, a1);
                acc[0][0] += a0;
                acc[0][1] += a1;
            }
        };
        // r[p][o] = sum_t a[p][o][t] * pl[o][t] for SIZE planes of the operand, over which the thread keeps each plaintext pair in registers
        template <unsigned SIZE>
        struct DotPlainTerm : Products
        {
            // (waves: the 128-, 72- and 96-register brackets.  Left to itself the scheduler trades the 7 waves of two planes for 4)
            static constexpr unsigned kOut = SIZE, kFlush = kDotFlush, kWaves = SIZE == 3 ? 4 : SIZE == 2 ? 7 : 5;
            static __device__ __forceinline__ void add(Acc (&acc)[kOut][2], const uint64_t *ap, const uint64_t *pp, const ReduceGeom &g)
            {
                uint64_t p0, p1;
                ld2<true>(pp, p0, p1);
#pragma unroll
                for (unsigned p = 0; p < SIZE; p++)
                {
                    uint64_t a0, a1;
                    ld2<true>(ap + p * g.a_plane, a0, a1);
                    mac128(acc[p][0], a0, p0);
                    mac128(acc[p][1], a1, p1);
                }
            }
        };
        // ciphertext x ciphertext, the size-2 x size-2 tensor product: c0 += x0 y0, c1 += x0 y1 + x1 y0, c2 += x1 y1 per item.
        // SQUARE: y is x - two loads per item, and the middle sum takes the one product x0 x1 twice (the same integer as x0 y1 + x1 y0)
        template <bool SQUARE>
        struct DotItemsTerm : Products
        {
            static constexpr unsigned kOut = 3, kFlush = kDotItemsFlush, kWaves = 4;
            static __device__ __forceinline__ void add(Acc (&acc)[kOut][2], const uint64_t *xp, const uint64_t *yp, const ReduceGeom &g)
            {
                uint64_t x0[2], x1[2];
                ld2<true>(xp, x0[0], x0[1]);
                ld2<true>(xp + g.a_plane, x1[0], x1[1]);
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
                    ld2<true>(yp + g.b_plane, y1[0], y1[1]);
                    for (unsigned l = 0; l < 2; l++)
                    {
                        mac128(acc[0][l], x0[l], y0[l]);
                        mac128(acc[1][l], x0[l], y1[l]);
                        mac128(acc[1][l], x1[l], y0[l]);
                        mac128(acc[2][l], x1[l], y1[l]);
                    }
                }
            }
        };

        // waves per SIMD a kernel is built for: its term's - except on the per-lane walk, which exists for the rings below N = 128 and
        // keeps a term index, two list pointers and two more addresses per lane: at the 7 waves of DotPlainTerm<2> (72 registers) it
        // spills, so it is built for 5 waves at most (96 registers; that term takes 90 there, and spills again at 4 and at 6)
        template <class Term, class Walk>
        constexpr unsigned walk_waves()
        {
            if constexpr (Walk::kMapped)
                return !Walk::kUniform && Term::kWaves > 5 ? 5 : Term::kWaves;
            else
                return Term::kWaves;
        }

        // FINAL: the result is the ciphertext (written once: non-temporal) and not scratch that the next launch reads
        template <class Term, bool FINAL, class Walk>
        __global__ void __launch_bounds__(kBlock, (walk_waves<Term, Walk>())) reduce_items_kernel(const ModDesc *mods, const uint64_t *a, const uint64_t *b, uint64_t *dst,
                                                                      ReduceGeom g, Walk walk)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.pairs)
                return;
            const size_t i = 2 * w, j = i & ((size_t(1) << g.n_log) - 1);
            unsigned row = (unsigned)(i >> g.n_log); // (p * out_items + o) * K + k
            if constexpr (Walk::kMapped)
            {
                if (Walk::kUniform)
                    row = SHL_UNIFORM(row);
            }
            const unsigned k = row % g.K, po = row / g.K, o = po % g.out_items, p = po / g.out_items;
            const ModDesc md = mods[k];
            unsigned t0, t1;
            size_t inner; // component k, coefficient j
            const uint64_t *ap;
            const typename Term::Second *bp;
            if constexpr (Walk::kMapped)
            {
                // the slice's part of row o: [off + s * per_slice, min(off + len, off + (s + 1) * per_slice)), empty past the row's end
                const unsigned off = Walk::ld(walk.off, o), len = Walk::ld(walk.off, o + 1) - off;
                const unsigned s0 = blockIdx.y * g.per_slice, r0 = s0 < len ? s0 : len;
                t0 = off + r0;
                t1 = len - r0 < g.per_slice ? off + len : t0 + g.per_slice;
                inner = ((size_t)k << g.n_log) + j;
                ap = a + p * g.a_plane + inner; // item 0: a term adds its item number times the words of an item
                bp = Term::second_base(b, p, k, inner, g);
            }
            else
            {
                t0 = blockIdx.y * g.per_slice;
                t1 = g.terms - t0 < g.per_slice ? g.terms : t0 + g.per_slice;
                inner = ((size_t)k << g.n_log) + j;
                const size_t first = o * g.item + t0 * g.term + inner; // output item o, term t0, component k, coefficient j
                ap = a + p * g.a_plane + first;
                bp = Term::second_base(b, p, k, first, g);
            }
            const size_t step = Walk::kMapped ? 0 : g.term; // consecutive items: the pointers walk; a map: they stay at item 0
            uint64_t tot[Term::kOut][2] = {};
            for (unsigned t = t0; t < t1;)
            {
                const unsigned end = t1 - t < Term::kFlush ? t1 : t + Term::kFlush;
                typename Term::Acc acc[Term::kOut][2] = {};
#pragma unroll Term::kUnroll
                for (; t < end; t++, ap += step, bp += step)
                {
                    if constexpr (Walk::kMapped) // g.term: the words of one item, below 2^32
                        Term::add(acc, ap + (size_t)Walk::ld(walk.first, t) * (unsigned)g.term, Term::second_at(bp, Walk::ld(walk.second, t), g), g);
                    else
                        Term::add(acc, ap, bp, g);
                }
                for (unsigned q = 0; q < Term::kOut; q++)
                    for (unsigned l = 0; l < 2; l++)
                        tot[q][l] = add_mod(tot[q][l], Term::reduce(acc[q][l], md), md.q);
            }
            uint64_t *d = dst + blockIdx.y * g.dst_slice + p * g.dst_plane + (((size_t)o * g.K) << g.n_log) + inner;
            for (unsigned q = 0; q < Term::kOut; q++)
            {
                if (FINAL)
                    st2_nt(d + q * g.dst_plane, tot[q][0], tot[q][1]);
                else
                    st2(d + q * g.dst_plane, tot[q][0], tot[q][1]);
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

        template <class Term, class Walk>
        hipError_t launch_walk(const ModDesc *mods, const uint64_t *a, const uint64_t *b, uint64_t *dst, const ReduceGeom &g, unsigned slices,
                               bool final, hipStream_t s, const Walk &walk)
        {
            unsigned blocks;
            if (!flat_grid(g.pairs, g.n_log, blocks))
                return hipErrorInvalidValue;
            if (final)
                hipLaunchKernelGGL((reduce_items_kernel<Term, true, Walk>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, a, b, dst, g, walk);
            else if constexpr (Term::kOperands)
                hipLaunchKernelGGL((reduce_items_kernel<Term, false, Walk>), dim3(blocks, slices), dim3(kBlock), 0, s, mods, a, b, dst, g, walk);
            else
                return hipErrorInvalidValue; // the slices are added into the result and nowhere else
            return hipGetLastError();
        }
        // the one launch: the walk picks the kernel's mode - consecutive groups, or a map read per wave (N >= 128) or per lane
        template <class Term>
        hipError_t launch_reduce(const ModDesc *mods, const uint64_t *a, const uint64_t *b, uint64_t *dst, const ReduceGeom &g, unsigned slices,
                                 bool final, hipStream_t s, const ItemWalk &walk)
        {
            if constexpr (Term::kOperands)
            {
                if (walk.mapped() && g.n_log >= 7)
                    return launch_walk<Term>(mods, a, b, dst, g, slices, final, s, MappedWalk<true>{ walk.offsets, walk.first, walk.second });
                if (walk.mapped())
                    return launch_walk<Term>(mods, a, b, dst, g, slices, final, s, MappedWalk<false>{ walk.offsets, walk.first, walk.second });
            }
            else if (walk.mapped())
                return hipErrorInvalidValue; // slice scratch is consecutive
            return launch_walk<Term>(mods, a, b, dst, g, slices, final, s, ConsecutiveWalk{});
        }

        // the second launch of a cut: r [size][out_items][K][N] (planes r_stride words apart) = the sum of scratch [slices][size][out_items][K][N]
        hipError_t sum_slices(const ModDesc *mods, const uint64_t *scratch, uint64_t *r, size_t r_stride, unsigned size, unsigned n_log, unsigned K,
                              size_t out_items, unsigned slices, hipStream_t s)
        {
            const size_t words = (size_t)K << n_log, out_plane = out_items * words;
            const ReduceGeom c{ out_plane, 0, words, size * out_plane, r_stride, 0, size * out_plane / 2, (unsigned)out_items, slices, slices, n_log, K };
            return launch_reduce<SumTerm<false>>(mods, scratch, scratch, r, c, 1, true, s, ItemWalk(slices));
        }

        // The host path of every reduction: r [size][out_items][K][N] (planes r_stride words apart) from operands whose planes are
        // a_plane / b_plane words apart and whose items are [K][N] blocks, the terms of an output item being what `walk` says.
        // launch(g, dst, slices, final) starts the reduction's own kernels over grid_planes planes per launch; with slices > 1 (a cut
        // of the longest row) they fill scratch [slices][size][out_items][K][N] and the sum of the slices follows.
        template <class Launch>
        hipError_t reduce_items(const ModDesc *mods, size_t a_plane, size_t b_plane, uint64_t *r, size_t r_stride, unsigned size,
                                unsigned grid_planes, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices,
                                uint64_t *scratch, hipStream_t s, Launch launch)
        {
            const size_t words = (size_t)K << n_log, out_plane = out_items * words, group = walk.longest;
            if (!size || !out_plane || !group)
                return hipSuccess;
            unsigned per_slice;
            if (!cut(group, slices, per_slice) || out_items > 0xffffffffu || (slices > 1 && !scratch) || (walk.mapped() && words > 0xffffffffu))
                return hipErrorInvalidValue;
            const bool final = slices == 1;
            const ReduceGeom g{ a_plane, b_plane, walk.mapped() ? 0 : group * words, words, final ? r_stride : out_plane, final ? 0 : size * out_plane,
                                grid_planes * out_plane / 2, (unsigned)out_items, walk.mapped() ? 0u : (unsigned)group, per_slice, n_log, K };
            const hipError_t e = launch(g, final ? r : scratch, slices, final);
            if (e != hipSuccess || final)
                return e;
            return sum_slices(mods, scratch, r, r_stride, size, n_log, K, out_items, slices, s);
        }

        // ---- the tiled products: r[p][i][j] = sum_t x[i][t] * y[p][t][j] over a rows x inner matrix x (ciphertexts, plaintexts or
        // scalar weights; item (i, t) at i * inner + t) and an inner x cols matrix y of ciphertext items.  One thread = W adjacent
        // words of one prime for a TILE of TR consecutive output rows x TC consecutive output columns: per t it loads the TR items
        // of x and the TC items of y once and uses them for all TR x TC outputs, which a kernel of one output per thread cannot do.
        // The grid is flat over (plane, row tile, column tile, prime, word), slices of the inner index in y.  The layouts of y and
        // of the result are two strides each, so [inner][cols] / [cols][inner] and [rows][cols] / [cols][rows] are one kernel.
        // Items are numbered arithmetically: there are no lists to read.
        // The accumulators are U128 and carry the running total themselves: a flush replaces the sum by its canonical residue, and
        // the next run of terms is added on top of that residue - which fits, see the static_assert - so no second set of totals
        // is kept in registers.
        // Partial tiles at the right and bottom edges: dead rows and columns are neither loaded nor stored (FULL = false).
        // What differs between the products is the BODY (matmul_words_body with its term, matmul_scalars_rows); the geometry, the
        // prologue (TileThread), the launch (launch_tiled), the thread count (tiled_threads), the tile ids (decode_tile) and the
        // host path (tiled_reduce) exist once.
        static_assert((unsigned __int128)kDotFlush * ((uint64_t(1) << kPrimeBits) - 1) * ((uint64_t(1) << kPrimeBits) - 1) <=
                          ~(unsigned __int128)0 - ((uint64_t(1) << kPrimeBits) - 1),
                      "a canonical residue plus kDotFlush products of words below 2^60 must fit 128 bits");
        // strides in words.  A row of the grid is ((p * row_tiles + row tile) * col_tiles + col tile) * K + k
        struct TileGeom
        {
            size_t x_plane;              // words between the two planes of an x item (ciphertext x ciphertext; otherwise 0)
            size_t y_plane;              // words between two planes of y
            size_t y_term, y_col;        // words from y item (t, j) to (t + 1, j) / to (t, j + 1): the layout of y
            size_t r_row, r_col;         // words from result item (i, j) to (i + 1, j) / to (i, j + 1): the layout of the result
            size_t dst_plane, dst_slice; // result word of (slice s, plane p): s * dst_slice + p * dst_plane
            size_t threads;              // grid planes * row_tiles * col_tiles * K * N / W; 0: a launch that tiled_threads refuses
            unsigned rows, inner, cols;  // of the product
            unsigned row_tiles, col_tiles; // ceil(rows / TR), ceil(cols / TC)
            unsigned per_slice;          // slice s adds the t in [s * per_slice, min(inner, (s + 1) * per_slice))
            unsigned n_log, K;
        };
        // where a thread is: its prime k, grid plane p, the tile's first row i0 and column j0 with the live rows and columns from
        // there, the slice's terms [t0, t1) and the word of (component k, coefficient j) inside an item.
        // UNIFORM (valid from N = 128 on): a wave covers 128 consecutive words and never leaves its grid row, so the row number is
        // moved to an SGPR and everything derived from it is uniform.  Below N = 128 the lanes of a wave sit in different rows.
        struct TileThread
        {
            unsigned k, p, i0, j0, live_r, live_c, t0, t1;
            size_t word;
            // of thread w < g.threads of the flat grid
            template <unsigned TR, unsigned TC, unsigned W, bool UNIFORM>
            static __device__ __forceinline__ TileThread at(const TileGeom &g, size_t w)
            {
                const size_t i = W * w, j = i & ((size_t(1) << g.n_log) - 1);
                unsigned row = (unsigned)(i >> g.n_log);
                if (UNIFORM)
                    row = SHL_UNIFORM(row);
                const unsigned tile = row / g.K, pr = tile / g.col_tiles;
                TileThread th;
                th.k = row % g.K;
                th.p = pr / g.row_tiles;
                th.i0 = pr % g.row_tiles * TR;
                th.j0 = tile % g.col_tiles * TC;
                th.live_r = g.rows - th.i0 < TR ? g.rows - th.i0 : TR;
                th.live_c = g.cols - th.j0 < TC ? g.cols - th.j0 : TC;
                th.t0 = blockIdx.y * g.per_slice;
                th.t1 = g.inner - th.t0 < g.per_slice ? g.inner : th.t0 + g.per_slice;
                th.word = ((size_t)th.k << g.n_log) + j;
                return th;
            }
        };

        // ---- word plaintexts: x items are [K][N] words like y's.  NT: the operand loads carry the non-temporal hint.  Unlike in
        // the other reductions an operand word is used by several tiles (a row of x by every column tile and, for plaintexts, by
        // every plane; a column of y by every row tile), so both forms are built and were measured (profiles/matmul_items.txt,
        // profiles/matmul_plain_items.txt): the hint wins where the operands come from HBM.
        template <unsigned W, bool NT>
        __device__ __forceinline__ void ldw(const uint64_t *p, uint64_t (&v)[W])
        {
            if constexpr (W == 2)
                ld2<NT>(p, v[0], v[1]);
            else
            {
#if defined(__HIP_DEVICE_COMPILE__)
                v[0] = NT ? __builtin_nontemporal_load(p) : *p;
#else
                v[0] = *p;
#endif
            }
        }
        template <unsigned W, bool FINAL>
        __device__ __forceinline__ void stw(uint64_t *p, const U128 (&v)[W])
        {
            if constexpr (W == 2)
            {
                if (FINAL)
                    st2_nt(p, v[0].lo, v[1].lo);
                else
                    st2(p, v[0].lo, v[1].lo);
            }
            else
            {
#if defined(__HIP_DEVICE_COMPILE__)
                if (FINAL)
                    __builtin_nontemporal_store(v[0].lo, p);
                else
#endif
                    *p = v[0].lo;
            }
        }
        // The terms of the word-plaintext products.  A term has kPlanesX / kPlanesY planes loaded per x / y item, kOut sums per
        // tile cell, kFlush terms between two reductions and mac(): add word l of the term of one cell to the cell's sums.
        // ciphertext matrix x ciphertext matrix (batch_reduce_kernels.h: k_matmul_items), DotItemsTerm<false>'s term: per t a tile
        // loads both planes of its TR x-items and TC y-items - 2 (TR + TC) plane-items per TR TC terms where one output per thread
        // reads 4 per term
        struct MatmulItemsTerm
        {
            static constexpr unsigned kPlanesX = 2, kPlanesY = 2, kOut = 3, kFlush = kDotItemsFlush;
            template <unsigned W>
            static __device__ __forceinline__ void mac(U128 (&acc)[kOut][W], const uint64_t (&x)[kPlanesX][W], const uint64_t (&y)[kPlanesY][W], unsigned l)
            {
                mac128(acc[0][l], x[0][l], y[0][l]);
                mac128(acc[1][l], x[0][l], y[1][l]);
                mac128(acc[1][l], x[1][l], y[0][l]);
                mac128(acc[2][l], x[1][l], y[1][l]);
            }
        };
        // plaintext matrix x ciphertext matrix (batch_reduce_kernels.h: k_matmul_plain_items), DotPlainTerm's term for ONE plane:
        // the planes are in the grid, so any size is one launch.  (TP + TC) plane-items per TP TC terms where one output per
        // thread reads (size + 1) / size per term
        struct MatmulPlainTerm
        {
            static constexpr unsigned kPlanesX = 1, kPlanesY = 1, kOut = 1, kFlush = kDotFlush;
            template <unsigned W>
            static __device__ __forceinline__ void mac(U128 (&acc)[kOut][W], const uint64_t (&x)[kPlanesX][W], const uint64_t (&y)[kPlanesY][W], unsigned l)
            {
                mac128(acc[0][l], x[0][l], y[0][l]);
            }
        };
        // The built tiles: words per thread and the waves per SIMD the allocator is held to (profiles/matmul_items.txt and
        // profiles/matmul_plain_items.txt have the registers; no tile uses scratch memory at these).
        // Ciphertext x ciphertext: a thread holds a 16-byte pair, as in the other kernels, while its 3 TR TC W sums of four
        // registers and the operands of a term fit the 168 registers of three waves: 2 x 2 with pairs is 96 + 32 (162 allocated;
        // one word per thread takes 144, and spills at the 128 of four waves).  2 x 4 holds one word.
        // Plaintext x ciphertext: a sum is four registers and a 64 x 64 multiply-accumulate takes about ten more, so from 2 x 4 on
        // a thread holds one word: 2 x 4 takes 90 registers (with a pair, or at six waves, it spills), 4 x 4 134 (it spills at the
        // 128 of four waves) and 4 x 8 needs 287 - the 32 past 255 are accumulation registers, which only one wave per SIMD can
        // have; at two waves it spills 124 bytes per lane
        template <class Term, unsigned TR, unsigned TC>
        struct Tile;
        template <unsigned WORDS, unsigned WAVES>
        struct TileOf
        {
            static constexpr unsigned kWords = WORDS, kWaves = WAVES;
        };
        // clang-format off
        template <> struct Tile<MatmulItemsTerm, 1, 1> : TileOf<2, 5> {};
        template <> struct Tile<MatmulItemsTerm, 2, 2> : TileOf<2, 3> {};
        template <> struct Tile<MatmulItemsTerm, 2, 4> : TileOf<1, 3> {};
        template <> struct Tile<MatmulPlainTerm, 1, 1> : TileOf<2, 8> {};
        template <> struct Tile<MatmulPlainTerm, 2, 4> : TileOf<1, 5> {};
        template <> struct Tile<MatmulPlainTerm, 4, 4> : TileOf<1, 3> {};
        template <> struct Tile<MatmulPlainTerm, 4, 8> : TileOf<1, 1> {};
        // clang-format on
        template <class Term, unsigned TR, unsigned TC, bool NT, bool FINAL, bool FULL>
        __device__ __forceinline__ void matmul_words_body(const ModDesc &md, const uint64_t *xp, const uint64_t *yp, uint64_t *d, const TileGeom &g,
                                                          const TileThread &th)
        {
            constexpr unsigned W = Tile<Term, TR, TC>::kWords;
            const size_t words = (size_t)g.K << g.n_log, x_row = (size_t)g.inner * words; // between two items / two rows of x
            const unsigned t1 = th.t1, live_r = th.live_r, live_c = th.live_c;
            U128 acc[TR][TC][Term::kOut][W] = {};
            for (unsigned t = th.t0; t < t1;)
            {
                const unsigned end = t1 - t < Term::kFlush ? t1 : t + Term::kFlush;
                for (; t < end; t++, xp += words, yp += g.y_term)
                {
                    uint64_t x[TR][Term::kPlanesX][W], y[TC][Term::kPlanesY][W];
#pragma unroll
                    for (unsigned r = 0; r < TR; r++)
                        if (FULL || r < live_r)
                            for (unsigned q = 0; q < Term::kPlanesX; q++)
                                ldw<W, NT>(xp + r * x_row + q * g.x_plane, x[r][q]);
#pragma unroll
                    for (unsigned c = 0; c < TC; c++)
                        if (FULL || c < live_c)
                            for (unsigned q = 0; q < Term::kPlanesY; q++)
                                ldw<W, NT>(yp + c * g.y_col + q * g.y_plane, y[c][q]);
#pragma unroll
                    for (unsigned r = 0; r < TR; r++)
#pragma unroll
                        for (unsigned c = 0; c < TC; c++)
                            if (FULL || (r < live_r && c < live_c))
                                for (unsigned l = 0; l < W; l++)
                                    Term::mac(acc[r][c], x[r], y[c], l);
                }
#pragma unroll
                for (unsigned r = 0; r < TR; r++)
#pragma unroll
                    for (unsigned c = 0; c < TC; c++)
                        if (FULL || (r < live_r && c < live_c))
                            for (unsigned q = 0; q < Term::kOut; q++)
                                for (unsigned l = 0; l < W; l++)
                                    acc[r][c][q][l] = U128{ barrett128(acc[r][c][q][l].lo, acc[r][c][q][l].hi, md), 0 };
            }
#pragma unroll
            for (unsigned r = 0; r < TR; r++)
#pragma unroll
                for (unsigned c = 0; c < TC; c++)
                    if (FULL || (r < live_r && c < live_c))
                        for (unsigned q = 0; q < Term::kOut; q++)
                            stw<W, FINAL>(d + r * g.r_row + c * g.r_col + q * g.dst_plane, acc[r][c][q]);
        }
        template <class Term, unsigned TR, unsigned TC, bool NT, bool FINAL>
        __global__ void __launch_bounds__(kBlock, (Tile<Term, TR, TC>::kWaves)) matmul_words_kernel(const ModDesc *mods, const uint64_t *x, const uint64_t *y, uint64_t *dst, TileGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.threads)
                return;
            const TileThread th = TileThread::at<TR, TC, Tile<Term, TR, TC>::kWords, false>(g, w);
            const ModDesc md = mods[th.k];
            const size_t words = (size_t)g.K << g.n_log;
            const uint64_t *xp = x + ((size_t)th.i0 * g.inner + th.t0) * words + th.word;            // item (i0, t0)
            const uint64_t *yp = y + th.p * g.y_plane + th.t0 * g.y_term + th.j0 * g.y_col + th.word; // plane p of item (t0, j0)
            uint64_t *d = dst + blockIdx.y * g.dst_slice + th.p * g.dst_plane + th.i0 * g.r_row + th.j0 * g.r_col + th.word;
            if (th.live_r == TR && th.live_c == TC)
                matmul_words_body<Term, TR, TC, NT, FINAL, true>(md, xp, yp, d, g, th);
            else
                matmul_words_body<Term, TR, TC, NT, FINAL, false>(md, xp, yp, d, g, th);
        }
        // the kernels of a tile by (NT, FINAL): what launch_tiled starts
        template <class Term, unsigned TR, unsigned TC>
        struct WordsFamily
        {
            template <bool NT, bool FINAL>
            static constexpr auto kernel = &matmul_words_kernel<Term, TR, TC, NT, FINAL>;
        };
        // the tiles the library runs with and whether their operand loads are non-temporal: the fastest of the built ones at
        // N = 65536, 8 x 16 x 8 (tools/matmul_items_rate.py and tools/matmul_plain_items_rate.py measure every tile both ways;
        // DESIGN.md 8.7 and 8.8 have the tables).  Where the operands come from HBM the hint wins by 4 - 8 % (ciphertexts) and
        // 1 - 2 % (plaintexts), and loses 8 - 15 % where they fit the caches (N = 8192); the plaintexts' 4 x 8 at its one wave per
        // SIMD is 15 - 17 % behind 4 x 4 there
        constexpr unsigned kMatmulTile = matmul_items_tile_id(2, 4), kMatmulPlainTile = matmul_items_tile_id(4, 4);
        constexpr bool kMatmulNonTemporal = true, kMatmulPlainNonTemporal = true;

        // ---- scalar weights (batch_reduce_kernels.h: k_matmul_scalars, and k_dot_scalars, which is its one column): the x item of
        // term (i, t) is ONE value per prime.  One thread = one 16-byte pair of one plane, one prime and one output COLUMN for a
        // tile of R consecutive output rows: the operand pair of (t, j) is loaded once and used for R x 2 products, so the operand
        // crosses HBM once per tile of rows and not once per row.
        // UNIFORM (N >= 128): the R weights of a term are scalar loads through the constant address space - SGPRs, not VGPRs, and
        // uniform trip counts.  The weights are therefore read through the constant cache: they must have been WRITTEN BY
        // SOMETHING EARLIER ON THE STREAM (a copy, a previous kernel), as the lists of an item map.  Below N = 128 the loads are
        // per lane.
        // Two forms of the weights:
        //   wide    [rows * inner][K] 64-bit words, weight (i, t) of prime q at (i * inner + t) * K + q: a 64 x 64 -> 128 multiply
        //           per product and the products' flush interval, kDotFlush.
        //   narrow  [rows * inner] signed 32-bit integers, one for all primes.  The weight w is used BIASED, u = w + 2^31 in
        //           [0, 2^32) (the sign bit flipped): sum_t a_t w_t = sum_t a_t u_t - 2^31 sum_t a_t.  Both sums are unsigned and
        //           exact; the second does not depend on the output row, so a thread keeps one per word of its pair and not one per
        //           row.  A product a u is two 32 x 32 -> 64 multiplies (the halves of a) where the wide form's compiles to six multiply
        //           instructions (four v_mad_u64_u32, two v_mul).  At a flush
        //           the total becomes  (P mod q) - (2^31 mod q) (S mod q)  mod q, the canonical residue of sum_t a_t w_t.
        // kNarrowFlush terms between two reductions.  Bound (the widest prime the library admits is below 2^60, so a canonical
        // word is at most 2^60 - 1; w = -2^31 gives u = 0 and w = 2^31 - 1 the largest u = 2^32 - 1, so every u is covered):
        //   P <= (q - 1) + T (2^60 - 1)(2^32 - 1) < 2^60 + T 2^92,   S <= T (2^60 - 1) < T 2^60
        // both below 2^128 for T <= 2^35.  The inner index is below 2^32, so the sums could not overflow at all; the interval is
        // kept far below the bound so that the loop is the wide form's and its boundary is met by tests of ordinary size - one
        // reduction of R + 1 sums per 1024 terms costs nothing measurable.
        constexpr unsigned kNarrowFlush = 1u << 10;
        static_assert((unsigned __int128)kNarrowFlush * ((uint64_t(1) << kPrimeBits) - 1) * 0xffffffffu <=
                          ~(unsigned __int128)0 - ((uint64_t(1) << kPrimeBits) - 1),
                      "a canonical residue plus kNarrowFlush products of a word below 2^60 and a biased 32-bit weight must fit 128 bits");
        // acc += a u for a canonical word a and a 32-bit u.  Written on the 128-bit integer type: the product becomes the two
        // 32 x 32 -> 64 multiply-adds of the halves of a and the sum one chain of four adds with carry, 7 vector instructions per
        // product where the same sum through add128's comparison takes 11
        __device__ __forceinline__ void mac_narrow(U128 &acc, uint64_t a, uint32_t u)
        {
            const unsigned __int128 sum = ((unsigned __int128)acc.hi << 64 | acc.lo) + (unsigned __int128)a * u;
            acc.lo = (uint64_t)sum;
            acc.hi = (uint64_t)(sum >> 64);
        }
        // waves per SIMD the allocator is held to (profiles/matmul_scalars.txt and profiles/dot_scalars.txt have the registers: no
        // kernel uses scratch memory at these, and the allocator stays below them: 62 - 72 registers at four rows, 80 - 106 at
        // eight).  The per-lane kernels keep a weight address per lane and the narrow form two more sums.  Two rows are built for
        // the one-column product only (the sweep of tools/dot_scalars_rate.py)
        template <unsigned R, bool UNIFORM>
        constexpr unsigned matmul_scalars_waves()
        {
            return R == 2 ? (UNIFORM ? 8 : 5) : R == 4 ? 6 : 4;
        }
        template <unsigned R, bool NARROW, bool UNIFORM, bool FINAL, bool FULL>
        __device__ __forceinline__ void matmul_scalars_rows(const ModDesc &md, const uint64_t *ap, const void *weights, uint64_t *d, const TileGeom &g,
                                                            const TileThread &th)
        {
            using Word = std::conditional_t<NARROW, uint32_t, uint64_t>;
            constexpr unsigned kFlush = NARROW ? kNarrowFlush : kDotFlush;
            // weight (i0, t0) [of prime k]; words from a term to the next and from a row to the next
            const size_t first = (size_t)th.i0 * g.inner + th.t0, step = NARROW ? 1 : g.K, row_words = (size_t)g.inner * step;
            const Word *wp = static_cast<const Word *>(weights) + (NARROW ? first : first * g.K + th.k);
            const uint64_t bias = NARROW ? barrett64(uint64_t(1) << 31, md) : 0; // 2^31 mod q
            const unsigned t1 = th.t1, live = th.live_r;
            U128 acc[R][2] = {};
            for (unsigned t = th.t0; t < t1;)
            {
                const unsigned end = t1 - t < kFlush ? t1 : t + kFlush;
                U128 plain[2] = {}; // narrow: the sum of the operand words themselves
                for (; t < end; t++, ap += g.y_term, wp += step)
                {
                    uint64_t a0, a1;
                    ld2<true>(ap, a0, a1);
                    if (NARROW)
                    {
                        add128(plain[0], a0, 0);
                        add128(plain[1], a1, 0);
                    }
#pragma unroll
                    for (unsigned r = 0; r < R; r++)
                        if (FULL || r < live)
                        {
                            if constexpr (NARROW)
                            {
                                const uint32_t u = (UNIFORM ? SHL_UCONST32(wp)[r * row_words] : wp[r * row_words]) ^ 0x80000000u;
                                mac_narrow(acc[r][0], a0, u);
                                mac_narrow(acc[r][1], a1, u);
                            }
                            else
                            {
                                const uint64_t w = UNIFORM ? SHL_UCONST(wp)[r * row_words] : wp[r * row_words];
                                mac128(acc[r][0], a0, w);
                                mac128(acc[r][1], a1, w);
                            }
                        }
                }
                uint64_t less[2] = {}; // narrow: 2^31 times that sum
                if (NARROW)
                    for (unsigned l = 0; l < 2; l++)
                        less[l] = mul_mod(barrett128(plain[l].lo, plain[l].hi, md), bias, md);
#pragma unroll
                for (unsigned r = 0; r < R; r++)
                    if (FULL || r < live)
                        for (unsigned l = 0; l < 2; l++)
                            acc[r][l] = U128{ sub_mod(barrett128(acc[r][l].lo, acc[r][l].hi, md), less[l], md.q), 0 };
            }
#pragma unroll
            for (unsigned r = 0; r < R; r++)
                if (FULL || r < live)
                {
                    if (FINAL)
                        st2_nt(d + r * g.r_row, acc[r][0].lo, acc[r][1].lo);
                    else
                        st2(d + r * g.r_row, acc[r][0].lo, acc[r][1].lo);
                }
        }
        template <unsigned R, bool NARROW, bool UNIFORM, bool FINAL>
        __global__ void __launch_bounds__(kBlock, (matmul_scalars_waves<R, UNIFORM>())) matmul_scalars_kernel(const ModDesc *mods, const void *weights, const uint64_t *a, uint64_t *dst, TileGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.threads)
                return;
            const TileThread th = TileThread::at<R, 1, 2, UNIFORM>(g, w);
            const ModDesc md = mods[th.k];
            const uint64_t *ap = a + th.p * g.y_plane + th.t0 * g.y_term + th.j0 * g.y_col + th.word; // plane p of item (t0, j0)
            uint64_t *d = dst + blockIdx.y * g.dst_slice + th.p * g.dst_plane + th.i0 * g.r_row + th.j0 * g.r_col + th.word;
            if (th.live_r == R)
                matmul_scalars_rows<R, NARROW, UNIFORM, FINAL, true>(md, ap, weights, d, g, th);
            else
                matmul_scalars_rows<R, NARROW, UNIFORM, FINAL, false>(md, ap, weights, d, g, th);
        }
        // the kernels of a row tile by (UNIFORM, FINAL)
        template <unsigned R, bool NARROW>
        struct ScalarsFamily
        {
            template <bool UNIFORM, bool FINAL>
            static constexpr auto kernel = &matmul_scalars_kernel<R, NARROW, UNIFORM, FINAL>;
        };
        // the row tiles the library runs with (tools/dot_scalars_rate.py and tools/matmul_scalars_rate.py measure them; DESIGN.md
        // 8.6 and 8.9 have the tables).  Wide: the tiles are bound by the 64 x 64 multiplies (2.0 - 2.1 Tmac/s at N = 65536) and
        // R = 4 cuts small results less often.  Narrow: R = 4 is bound by the operand stream there, R = 8 is 8 - 10 % faster from
        // 8 rows on
        constexpr unsigned kRowTile = 4, kMatmulScalarsTile = 4, kMatmulScalarsNarrowTile = 8;

        // ---- 2-D convolution of scalar weights (batch_reduce_kernels.h: k_conv2d_scalars): the scalar-weights product with rows =
        // the output channels, cols = the output positions and inner = C * kh * kw, in the same grid, with the same prologue,
        // weights, accumulators and flushes.  What differs is where the operand of a term is: term t = (c * kh + dy) * kw + dx of
        // output position (y', x') is input item (c, y' sh + dy - ph, x' sw + dx - pw), three strides from the item of channel 0 at
        // the top left of the image, and a term outside the image is no term.  The result's layout is TileGeom's r_row (from a
        // channel to the next) and r_col (from a position to the next: a position is one index in both layouts).
        struct ConvGeom : TileGeom
        {
            size_t in_c, in_y, in_x; // words from input item (c, y, x) to (c + 1, y, x) / (c, y + 1, x) / (c, y, x + 1)
            size_t sh, sw;           // strides (1 where there is one output row / column: then no product with them matters)
            unsigned H, W, OW, kh, kw, ph, pw;
        };
        // one reduction of the tile's sums, which then carry their canonical residues; narrow: and of the plain sum, which restarts
        template <unsigned R, bool NARROW, bool FULL>
        __device__ __forceinline__ void scalars_flush(U128 (&acc)[R][2], U128 (&plain)[2], const ModDesc &md, uint64_t bias, unsigned live)
        {
            uint64_t less[2] = {}; // narrow: 2^31 times the sum of the operand words
            if (NARROW)
#pragma unroll
                for (unsigned l = 0; l < 2; l++)
                {
                    less[l] = mul_mod(barrett128(plain[l].lo, plain[l].hi, md), bias, md);
                    plain[l] = U128{ 0, 0 };
                }
#pragma unroll
            for (unsigned r = 0; r < R; r++)
                if (FULL || r < live)
#pragma unroll
                    for (unsigned l = 0; l < 2; l++)
                        acc[r][l] = U128{ sub_mod(barrett128(acc[r][l].lo, acc[r][l].hi, md), less[l], md.q), 0 };
        }
        // The in-image taps of an output position are a rectangle [dy0, dy1) x [dx0, dx1) of the kernel, the same for every channel
        // and computed once per thread (per wave when UNIFORM); the loop runs over the channels the slice [t0, t1) touches, the
        // live dy and, clipped to the slice, the live dx, whose operands are in_x words apart and whose weights are consecutive.
        // Nothing outside the batch is addressed: an operand pointer is formed for a live tap only.  `run` counts the executed
        // taps since the last reduction, so a run of taps ends where the sums could no longer take another one.
        // a: component k of plane p of input item (0, 0, 0); lane: the thread's words from there.  When UNIFORM the first is the
        // wave's and the walk from tap to tap is scalar arithmetic: a lane keeps one 32-bit offset, not the two pointers of the
        // per-lane walk.
        template <unsigned R, bool NARROW, bool NT, bool UNIFORM, bool FINAL, bool FULL>
        __device__ __forceinline__ void conv2d_scalars_rows(const ModDesc &md, const uint64_t *a, unsigned lane, const void *weights, uint64_t *d,
                                                            const ConvGeom &g, const TileThread &th)
        {
            using Word = std::conditional_t<NARROW, uint32_t, uint64_t>;
            constexpr unsigned kFlush = NARROW ? kNarrowFlush : kDotFlush;
            // weight (i0, term 0) [of prime k]; words from a term to the next and from a channel to the next
            const size_t step = NARROW ? 1 : g.K, row_words = (size_t)g.inner * step;
            const Word *wp = static_cast<const Word *>(weights) + (size_t)th.i0 * row_words + (NARROW ? 0 : th.k);
            const uint64_t bias = NARROW ? barrett64(uint64_t(1) << 31, md) : 0; // 2^31 mod q
            const unsigned live = th.live_r;
            // tap (dy, dx) of this position is input row y0 + dy - ph, column x0 + dx - pw (64 bits: H + ph may pass 2^32)
            const uint64_t y0 = th.j0 / g.OW * g.sh, x0 = th.j0 % g.OW * g.sw;
            const unsigned dy0 = y0 < g.ph ? (unsigned)(g.ph - y0) : 0, dy1 = (uint64_t)g.H + g.ph - y0 < g.kh ? (unsigned)((uint64_t)g.H + g.ph - y0) : g.kh;
            const unsigned dx0 = x0 < g.pw ? (unsigned)(g.pw - x0) : 0, dx1 = (uint64_t)g.W + g.pw - x0 < g.kw ? (unsigned)((uint64_t)g.W + g.pw - x0) : g.kw;
            const unsigned taps = g.kh * g.kw, c0 = th.t0 / taps, c1 = (th.t1 - 1) / taps; // (a slice is not empty)
            U128 acc[R][2] = {};
            U128 plain[2] = {}; // narrow: the sum of the operand words themselves
            unsigned run = 0;
            for (unsigned c = c0; c <= c1; c++)
                for (unsigned dy = dy0; dy < dy1; dy++)
                {
                    const unsigned base = (c * g.kh + dy) * g.kw; // term (c, dy, 0)
                    unsigned t = base + dx0 > th.t0 ? base + dx0 : th.t0;
                    const unsigned last = base + dx1 < th.t1 ? base + dx1 : th.t1;
                    if (t >= last)
                        continue;
                    const uint64_t *ap = a + c * g.in_c + (size_t)(y0 + dy - g.ph) * g.in_y + (size_t)(x0 + (t - base) - g.pw) * g.in_x;
                    const Word *w = wp + t * step;
                    while (t < last)
                    {
                        const unsigned end = last - t < kFlush - run ? last : t + (kFlush - run);
                        run += end - t;
                        for (; t < end; t++, ap += g.in_x, w += step)
                        {
                            uint64_t a0, a1;
                            ld2<NT>(ap + lane, a0, a1);
                            if (NARROW)
                            {
                                add128(plain[0], a0, 0);
                                add128(plain[1], a1, 0);
                            }
#pragma unroll
                            for (unsigned r = 0; r < R; r++)
                                if (FULL || r < live)
                                {
                                    if constexpr (NARROW)
                                    {
                                        const uint32_t u = (UNIFORM ? SHL_UCONST32(w)[r * row_words] : w[r * row_words]) ^ 0x80000000u;
                                        mac_narrow(acc[r][0], a0, u);
                                        mac_narrow(acc[r][1], a1, u);
                                    }
                                    else
                                    {
                                        const uint64_t v = UNIFORM ? SHL_UCONST(w)[r * row_words] : w[r * row_words];
                                        mac128(acc[r][0], a0, v);
                                        mac128(acc[r][1], a1, v);
                                    }
                                }
                        }
                        if (run == kFlush)
                        {
                            scalars_flush<R, NARROW, FULL>(acc, plain, md, bias, live);
                            run = 0;
                        }
                    }
                }
            scalars_flush<R, NARROW, FULL>(acc, plain, md, bias, live); // (of nothing but residues when the last run was full)
#pragma unroll
            for (unsigned r = 0; r < R; r++)
                if (FULL || r < live)
                {
                    if (FINAL)
                        st2_nt(d + r * g.r_row, acc[r][0].lo, acc[r][1].lo);
                    else
                        st2(d + r * g.r_row, acc[r][0].lo, acc[r][1].lo);
                }
        }
        // waves per SIMD the allocator is held to (profiles/conv2d_scalars.txt has the registers of every instantiation: none uses
        // scratch memory at these).  The wave-uniform kernels: the product's.  The per-lane kernels, which exist for the rings
        // below N = 128, keep the tap range, the term and two more addresses per lane and spill at the product's bounds
        template <unsigned R, bool NARROW, bool UNIFORM>
        constexpr unsigned conv2d_scalars_waves()
        {
            return !UNIFORM ? (R == 4 ? 4 : 3) : R == 4 ? matmul_scalars_waves<4, true>() : NARROW ? 4 : 5;
        }
        template <unsigned R, bool NARROW, bool NT, bool UNIFORM, bool FINAL>
        __global__ void __launch_bounds__(kBlock, (conv2d_scalars_waves<R, NARROW, UNIFORM>())) conv2d_scalars_kernel(const ModDesc *mods, const void *weights, const uint64_t *a, uint64_t *dst, ConvGeom g)
        {
            const size_t w = blockIdx.x * (size_t)kBlock + threadIdx.x;
            if (w >= g.threads)
                return;
            const TileThread th = TileThread::at<R, 1, 2, UNIFORM>(g, w); // i0: the tile's first output channel, j0: the output position
            const ModDesc md = mods[th.k];
            const unsigned lane = (unsigned)(th.word & ((size_t(1) << g.n_log) - 1)); // the coefficient
            const uint64_t *ap = a + th.p * g.y_plane + ((size_t)th.k << g.n_log); // component k of plane p of input item (0, 0, 0)
            uint64_t *d = dst + blockIdx.y * g.dst_slice + th.p * g.dst_plane + th.i0 * g.r_row + th.j0 * g.r_col + th.word;
            if (th.live_r == R)
                conv2d_scalars_rows<R, NARROW, NT, UNIFORM, FINAL, true>(md, ap, lane, weights, d, g, th);
            else
                conv2d_scalars_rows<R, NARROW, NT, UNIFORM, FINAL, false>(md, ap, lane, weights, d, g, th);
        }
        // the kernels of a row tile, a form and a hint by (UNIFORM, FINAL)
        template <unsigned R, bool NARROW, bool NT>
        struct ConvFamily
        {
            template <bool UNIFORM, bool FINAL>
            static constexpr auto kernel = &conv2d_scalars_kernel<R, NARROW, NT, UNIFORM, FINAL>;
        };
        // whether the library's operand loads carry the non-temporal hint (tools/conv2d_scalars_rate.py measures both; DESIGN.md
        // 8.11 has the table): not.  At N = 65536 the hint wins 1 % where 3 x 3 windows overlap over 8 channels and loses 5 - 11 % on
        // the 28 x 28 image under a 5 x 5 kernel, whose neighbouring outputs re-read an item while it is still cached; at
        // N = 8192, where the whole input fits the caches, it loses 4 - 9 % everywhere
        constexpr bool kConvNonTemporal = false;

        // ---- a sparse matrix of scalar weights (batch_reduce_kernels.h: k_dot_scalars_mapped): a Term of the reduce_items skeleton on
        // the mapped walks.  r[p][o] = sum_t const(w[second[t]]) a[p][first[t]]: the second operand of a term is not an item of
        // [K][N] words but ONE value per prime (wide: word k of weight second[t], at second[t] * K + k of [count][K] words) or one
        // signed 32-bit integer for all primes (narrow: at second[t] of [count]), indexed in 64 bits.  One thread = one pair of one
        // plane: the planes are in the grid as for the sum - the weight is a scalar, so nothing would be gained by keeping it in
        // registers over the planes as DotPlainTerm keeps its plaintext pair.
        // Wide: the products' accumulator and interval.  Narrow: the biased weight u = w + 2^31 and the two exact sums of the
        // scalar-weights product above (mac_narrow; sum a u and sum a), reduced once per kNarrowFlush terms to the same residue.
        // UNIFORM (the walk's: N >= 128): the row is the wave's, so a term is a chain of scalar loads - the two list entries, then
        // the weight, through the constant address space: the weights must have been WRITTEN BY SOMETHING EARLIER ON THE STREAM -
        // and one vector load of the operand pair.  The loop is unrolled kUnroll times, which lets the scheduler issue the list
        // and weight loads of the next terms ahead of the vector loads of these (profiles/dot_scalars_mapped.txt has what the ISA
        // shows).  Per lane below that.  The operand loads carry the non-temporal hint like the other mapped terms'.
        template <bool NARROW, bool UNIFORM>
        struct DotScalarsTerm
        {
            struct NarrowSums
            {
                U128 biased, plain; // sum a u, sum a
            };
            using Acc = std::conditional_t<NARROW, NarrowSums, U128>;
            using Second = std::conditional_t<NARROW, uint32_t, uint64_t>;
            static constexpr bool kOperands = true;
            // (waves: unrolled four times the wave-uniform kernels take 68 - 70 registers and spill at the 64 of eight waves; the
            // per-lane ones, unrolled twice, take 70 - 86: profiles/dot_scalars_mapped.txt.  None uses scratch memory at these)
            static constexpr unsigned kOut = 1, kFlush = NARROW ? kNarrowFlush : kDotFlush, kUnroll = UNIFORM ? 4 : 2, kWaves = UNIFORM ? 6 : 5;
            static __device__ __forceinline__ const Second *second_base(const uint64_t *weights, unsigned, unsigned k, size_t, const ReduceGeom &)
            {
                return reinterpret_cast<const Second *>(weights) + (NARROW ? 0 : k);
            }
            static __device__ __forceinline__ const Second *second_at(const Second *wp, unsigned weight, const ReduceGeom &g)
            {
                return wp + (NARROW ? (size_t)weight : (size_t)weight * g.K);
            }
            static __device__ __forceinline__ uint64_t reduce(const Acc &acc, const ModDesc &md)
            {
                if constexpr (NARROW)
                {
                    // sum a w = P - 2^31 S exactly, as sign and magnitude, and ONE reduction of the magnitude: P < 2^128 by
                    // kNarrowFlush's bound and 2^31 S < 2^31 2^10 2^60.  (scalars_flush reduces P and S apart and multiplies by
                    // 2^31 mod q: three reductions per word where rows are a handful of terms long and this is most of the work -
                    // at N = 8192 that form was 10 - 20 % behind DotPlainTerm on rows of 4 to 9 terms, profiles/dot_scalars_mapped.txt)
                    const unsigned __int128 p = (unsigned __int128)acc.biased.hi << 64 | acc.biased.lo;
                    const unsigned __int128 s = ((unsigned __int128)acc.plain.hi << 64 | acc.plain.lo) << 31;
                    const bool negative = p < s;
                    const unsigned __int128 magnitude = negative ? s - p : p - s;
                    const uint64_t r = barrett128((uint64_t)magnitude, (uint64_t)(magnitude >> 64), md);
                    return negative && r ? md.q - r : r;
                }
                else
                    return barrett128(acc.lo, acc.hi, md);
            }
            static __device__ __forceinline__ void add(Acc (&acc)[kOut][2], const uint64_t *ap, const Second *wp, const ReduceGeom &)
            {
                uint64_t a0, a1;
                ld2<true>(ap, a0, a1);
                if constexpr (NARROW)
                {
                    const uint32_t u = (UNIFORM ? *SHL_UCONST32(wp) : *wp) ^ 0x80000000u;
                    mac_narrow(acc[0][0].biased, a0, u);
                    mac_narrow(acc[0][1].biased, a1, u);
                    add128(acc[0][0].plain, a0, 0);
                    add128(acc[0][1].plain, a1, 0);
                }
                else
                {
                    const uint64_t w = UNIFORM ? *SHL_UCONST(wp) : *wp;
                    mac128(acc[0][0], a0, w);
                    mac128(acc[0][1], a1, w);
                }
            }
        };

        // ---- the built tiles of a product as a list, and the one dispatch on it: f(BuiltTile<TR, TC>{}) for the tile that is
        // TR x TC; false = not built
        template <unsigned TR, unsigned TC>
        struct BuiltTile
        {
            static constexpr unsigned kRows = TR, kCols = TC;
        };
        template <class... Tiles>
        struct BuiltTiles
        {
            template <class F>
            static bool with(unsigned tr, unsigned tc, F f)
            {
                return ((tr == Tiles::kRows && tc == Tiles::kCols && (f(Tiles{}), true)) || ...);
            }
        };
        using MatmulItemsTiles = BuiltTiles<BuiltTile<1, 1>, BuiltTile<2, 2>, BuiltTile<2, 4>>;
        using MatmulPlainTiles = BuiltTiles<BuiltTile<1, 1>, BuiltTile<2, 4>, BuiltTile<4, 4>, BuiltTile<4, 8>>;
        using MatmulScalarsTiles = BuiltTiles<BuiltTile<4, 1>, BuiltTile<8, 1>>;
        using DotScalarsTiles = BuiltTiles<BuiltTile<2, 1>, BuiltTile<4, 1>, BuiltTile<8, 1>>; // wide only
        // a tile id with the hint bits (batch_reduce_kernels.h) -> its shape (0: the library's), words per thread and hint
        // (neither bit: the library's); false = both hint bits, or a tile that is not built
        struct TileChoice
        {
            unsigned tr, tc, words;
            bool nt;
        };
        template <class Term, class Built>
        inline bool decode_tile(unsigned tile, unsigned library, bool library_nt, TileChoice &c)
        {
            const unsigned hint = tile & kMatmulItemsHintMask, shape = tile & ~kMatmulItemsHintMask ? tile & ~kMatmulItemsHintMask : library;
            c.tr = shape >> 8;
            c.tc = shape & 0xff;
            c.nt = hint ? hint == kMatmulItemsNonTemporal : library_nt;
            return hint != kMatmulItemsHintMask &&
                   Built::with(c.tr, c.tc, [&](auto t) { c.words = Tile<Term, decltype(t)::kRows, decltype(t)::kCols>::kWords; });
        }

        // threads of a tiled launch: one per W words of (grid plane, row tile, column tile, prime); 0 = a launch that is refused -
        // flat_grid's refusal, which counts pairs (rows of the grid are numbered in 32 bits); a thread of one word makes twice the
        // workgroups
        inline size_t tiled_threads(unsigned planes, size_t rows, size_t cols, unsigned n_log, unsigned K, unsigned tr, unsigned tc, unsigned words)
        {
            if (rows > 0xffffffffu || cols > 0xffffffffu)
                return 0;
            const size_t grid_rows = planes * ((rows + tr - 1) / tr) * ((cols + tc - 1) / tc) * K, threads = (grid_rows << n_log) / words;
            unsigned blocks;
            if (!flat_grid(threads * words / 2, n_log, blocks) || (threads + kBlock - 1) / kBlock > 0x7fffffffu)
                return 0;
            return threads;
        }
        // the one launch of the tiled kernels: Family::kernel<first, FINAL>, `first` being the family's own switch (NT, UNIFORM);
        // Geom: TileGeom, or what a family's kernels take in its place (ConvGeom)
        template <class Family, class X, class Geom>
        hipError_t launch_tiled(const ModDesc *mods, const X *x, const uint64_t *y, uint64_t *dst, const Geom &g, unsigned slices, bool first,
                                bool final, hipStream_t s)
        {
            if (!g.threads)
                return hipErrorInvalidValue;
            const dim3 grid((unsigned)((g.threads + kBlock - 1) / kBlock), slices), block(kBlock);
            const auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, mods, x, y, dst, g); };
            if (first)
                final ? go(Family::template kernel<true, true>) : go(Family::template kernel<true, false>);
            else
                final ? go(Family::template kernel<false, true>) : go(Family::template kernel<false, false>);
            return hipGetLastError();
        }
        // The host path of every tiled product: r [size][rows * cols][K][N] (planes r_stride words apart) from x, whose items have
        // planes x_plane words apart, and y, whose planes are y_plane words apart, in the layouts the flags name.  `threads` is
        // tiled_threads' count for the tile tr x tc.  launch(g, dst, slices, final) starts the product's kernel; with slices > 1 (a
        // cut of the inner index) it fills scratch [slices][size][rows * cols][K][N] and the sum of the slices follows.
        template <class Launch>
        hipError_t tiled_reduce(const ModDesc *mods, size_t x_plane, size_t y_plane, bool y_transposed, uint64_t *r, size_t r_stride, bool r_transposed,
                                unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols, unsigned tr, unsigned tc,
                                size_t threads, unsigned slices, uint64_t *scratch, hipStream_t s, Launch launch)
        {
            unsigned per_slice;
            const size_t words = (size_t)K << n_log;
            if (!size || !rows || !inner || !cols || !words || rows > 0xffffffffu || inner > 0xffffffffu || cols > 0xffffffffu ||
                rows * inner > 0xffffffffu || inner * cols > 0xffffffffu || rows * cols > 0xffffffffu || !cut(inner, slices, per_slice) ||
                (slices > 1 && !scratch))
                return hipErrorInvalidValue;
            const bool final = slices == 1;
            const size_t out_plane = rows * cols * words;
            const TileGeom g{ x_plane,
                              y_plane,
                              y_transposed ? words : cols * words,
                              y_transposed ? inner * words : words,
                              r_transposed ? words : cols * words,
                              r_transposed ? rows * words : words,
                              final ? r_stride : out_plane,
                              final ? 0 : size * out_plane,
                              threads,
                              (unsigned)rows,
                              (unsigned)inner,
                              (unsigned)cols,
                              (unsigned)((rows + tr - 1) / tr),
                              (unsigned)((cols + tc - 1) / tc),
                              per_slice,
                              n_log,
                              K };
            const hipError_t e = launch(g, final ? r : scratch, slices, final);
            if (e != hipSuccess || final)
                return e;
            return sum_slices(mods, scratch, r, r_stride, size, n_log, K, rows * cols, slices, s);
        }
        // the launch of a word-plaintext product with the tile decode_tile chose
        template <class Term, class Built>
        hipError_t launch_words(const ModDesc *mods, const uint64_t *x, const uint64_t *y, uint64_t *dst, const TileGeom &g, unsigned slices,
                                const TileChoice &c, bool final, hipStream_t s)
        {
            hipError_t e = hipErrorInvalidValue;
            Built::with(c.tr, c.tc, [&](auto t) {
                e = launch_tiled<WordsFamily<Term, decltype(t)::kRows, decltype(t)::kCols>>(mods, x, y, dst, g, slices, c.nt, final, s);
            });
            return e;
        }
        // k_matmul_scalars and k_dot_scalars: the tiled host path with the scalar-weights kernel of row tile R, one of Built's
        template <class Built>
        hipError_t scalars_reduce(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                  size_t r_stride, unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols,
                                  bool a_transposed, bool r_transposed, unsigned slices, uint64_t *scratch, unsigned R, hipStream_t s)
        {
            if (!Built::with(R, 1, [](auto) {}))
                return hipErrorInvalidValue;
            return tiled_reduce(mods, 0, a_stride, a_transposed, r, r_stride, r_transposed, size, n_log, K, rows, inner, cols, R, 1,
                                tiled_threads(size, rows, cols, n_log, K, R, 1, 2), slices, scratch, s,
                                [=](const TileGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                    hipError_t e = hipErrorInvalidValue;
                                    Built::with(R, 1, [&](auto t) {
                                        constexpr unsigned kR = decltype(t)::kRows;
                                        if constexpr (kR != 2) // two rows: the wide form only
                                        {
                                            if (narrow)
                                            {
                                                e = launch_tiled<ScalarsFamily<kR, true>>(mods, weights, a, dst, g, ns, n_log >= 7, final, s);
                                                return;
                                            }
                                        }
                                        e = launch_tiled<ScalarsFamily<kR, false>>(mods, weights, a, dst, g, ns, n_log >= 7, final, s);
                                    });
                                    return e;
                                });
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
    unsigned batch_reduce_slices(size_t threads, const ItemWalk &walk)
    {
        unsigned slices = batch_reduce_slices(threads, walk.mean), per_slice;
        cut(walk.longest, slices, per_slice); // mean <= longest: the slices of the mean row fit the longest one
        return slices;
    }

    hipError_t k_sum_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, uint64_t *r, size_t r_stride, unsigned size, unsigned n_log,
                           unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices, uint64_t *scratch, hipStream_t s)
    {
        return reduce_items(mods, a_stride, 0, r, r_stride, size, size, n_log, K, out_items, walk, slices, scratch, s,
                            [=](const ReduceGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                return launch_reduce<SumTerm<true>>(mods, a, a, dst, g, ns, final, s, walk);
                            });
    }

    hipError_t k_dot_plain_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride,
                                 unsigned size, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices,
                                 uint64_t *scratch, hipStream_t s)
    {
        return reduce_items(mods, a_stride, 0, r, r_stride, size, 1, n_log, K, out_items, walk, slices, scratch, s,
                            [=](const ReduceGeom &g, uint64_t *dst, unsigned ns, bool final) -> hipError_t {
                                // three planes at a time, then two or one: the plaintexts are read once for size <= 3
                                for (unsigned p = 0; p < size;)
                                {
                                    const unsigned take = std::min(3u, size - p);
                                    const uint64_t *ap = a + p * a_stride;
                                    uint64_t *dp = dst + p * g.dst_plane;
                                    const hipError_t e = take == 3   ? launch_reduce<DotPlainTerm<3>>(mods, ap, pl, dp, g, ns, final, s, walk)
                                                         : take == 2 ? launch_reduce<DotPlainTerm<2>>(mods, ap, pl, dp, g, ns, final, s, walk)
                                                                     : launch_reduce<DotPlainTerm<1>>(mods, ap, pl, dp, g, ns, final, s, walk);
                                    if (e != hipSuccess)
                                        return e;
                                    p += take;
                                }
                                return hipSuccess;
                            });
    }

    hipError_t k_dot_items(const ModDesc *mods, const uint64_t *x, size_t x_stride, const uint64_t *y, size_t y_stride, uint64_t *r,
                           size_t r_stride, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices,
                           uint64_t *scratch, hipStream_t s)
    {
        // the square: one operand and one list of items
        const bool square = x == y && x_stride == y_stride && walk.first == walk.second;
        return reduce_items(mods, x_stride, y_stride, r, r_stride, 3, 1, n_log, K, out_items, walk, slices, scratch, s,
                            [=](const ReduceGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                return square ? launch_reduce<DotItemsTerm<true>>(mods, x, y, dst, g, ns, final, s, walk)
                                              : launch_reduce<DotItemsTerm<false>>(mods, x, y, dst, g, ns, final, s, walk);
                            });
    }

    // the sum's geometry (the planes in the grid) with the scalar term on the map's walk: per wave from N = 128 on, per lane below
    hipError_t k_dot_scalars_mapped(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                    size_t r_stride, unsigned size, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk,
                                    unsigned slices, uint64_t *scratch, hipStream_t s)
    {
        if (!walk.mapped())
            return hipErrorInvalidValue; // consecutive items are k_dot_scalars'
        const uint64_t *w = static_cast<const uint64_t *>(weights);
        return reduce_items(mods, a_stride, 0, r, r_stride, size, size, n_log, K, out_items, walk, slices, scratch, s,
                            [=](const ReduceGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                const MappedWalk<true> wave{ walk.offsets, walk.first, walk.second };
                                const MappedWalk<false> lane{ walk.offsets, walk.first, walk.second };
                                if (n_log >= 7)
                                    return narrow ? launch_walk<DotScalarsTerm<true, true>>(mods, a, w, dst, g, ns, final, s, wave)
                                                  : launch_walk<DotScalarsTerm<false, true>>(mods, a, w, dst, g, ns, final, s, wave);
                                return narrow ? launch_walk<DotScalarsTerm<true, false>>(mods, a, w, dst, g, ns, final, s, lane)
                                              : launch_walk<DotScalarsTerm<false, false>>(mods, a, w, dst, g, ns, final, s, lane);
                            });
    }

    unsigned dot_scalars_row_tile()
    {
        return kRowTile;
    }
    size_t dot_scalars_threads(unsigned size, size_t rows, unsigned n_log, unsigned K, unsigned row_tile)
    {
        return tiled_threads(size, rows, 1, n_log, K, row_tile ? row_tile : kRowTile, 1, 2);
    }
    // k_matmul_scalars' wide form at one column: inner = batch, neither layout flag, weights = scalars
    hipError_t k_dot_scalars(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *scalars, uint64_t *r, size_t r_stride,
                             unsigned size, unsigned n_log, unsigned K, size_t rows, size_t batch, unsigned slices, uint64_t *scratch,
                             unsigned row_tile, hipStream_t s)
    {
        if (!size || !rows || !K || !batch)
            return hipSuccess;
        return scalars_reduce<DotScalarsTiles>(mods, scalars, false, a, a_stride, r, r_stride, size, n_log, K, rows, batch, 1, false, false, slices,
                                               scratch, row_tile ? row_tile : kRowTile, s);
    }

    void matmul_items_tile(unsigned &tile_rows, unsigned &tile_cols)
    {
        tile_rows = kMatmulTile >> 8;
        tile_cols = kMatmulTile & 0xff;
    }
    size_t matmul_items_threads(size_t rows, size_t cols, unsigned n_log, unsigned K, unsigned tile)
    {
        TileChoice c;
        if (!decode_tile<MatmulItemsTerm, MatmulItemsTiles>(tile, kMatmulTile, kMatmulNonTemporal, c))
            return 0;
        return tiled_threads(1, rows, cols, n_log, K, c.tr, c.tc, c.words);
    }
    hipError_t k_matmul_items(const ModDesc *mods, const uint64_t *x, size_t x_stride, const uint64_t *y, size_t y_stride, uint64_t *r,
                              size_t r_stride, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols, bool y_transposed,
                              unsigned slices, uint64_t *scratch, unsigned tile, hipStream_t s)
    {
        TileChoice c;
        if (!decode_tile<MatmulItemsTerm, MatmulItemsTiles>(tile, kMatmulTile, kMatmulNonTemporal, c))
            return hipErrorInvalidValue;
        // one grid plane: a thread forms the three result planes, dst_plane words apart
        return tiled_reduce(mods, x_stride, y_stride, y_transposed, r, r_stride, false, 3, n_log, K, rows, inner, cols, c.tr, c.tc,
                            tiled_threads(1, rows, cols, n_log, K, c.tr, c.tc, c.words), slices, scratch, s,
                            [=](const TileGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                return launch_words<MatmulItemsTerm, MatmulItemsTiles>(mods, x, y, dst, g, ns, c, final, s);
                            });
    }

    void matmul_plain_items_tile(unsigned &tile_rows, unsigned &tile_cols)
    {
        tile_rows = kMatmulPlainTile >> 8;
        tile_cols = kMatmulPlainTile & 0xff;
    }
    size_t matmul_plain_items_threads(unsigned size, size_t rows, size_t cols, unsigned n_log, unsigned K, unsigned tile)
    {
        TileChoice c;
        if (!decode_tile<MatmulPlainTerm, MatmulPlainTiles>(tile, kMatmulPlainTile, kMatmulPlainNonTemporal, c))
            return 0;
        return tiled_threads(size, rows, cols, n_log, K, c.tr, c.tc, c.words);
    }
    hipError_t k_matmul_plain_items(const ModDesc *mods, const uint64_t *pl, const uint64_t *a, size_t a_stride, uint64_t *r, size_t r_stride,
                                    unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols, bool a_transposed,
                                    bool r_transposed, unsigned slices, uint64_t *scratch, unsigned tile, hipStream_t s)
    {
        TileChoice c;
        if (!decode_tile<MatmulPlainTerm, MatmulPlainTiles>(tile, kMatmulPlainTile, kMatmulPlainNonTemporal, c))
            return hipErrorInvalidValue;
        return tiled_reduce(mods, 0, a_stride, a_transposed, r, r_stride, r_transposed, size, n_log, K, rows, inner, cols, c.tr, c.tc,
                            tiled_threads(size, rows, cols, n_log, K, c.tr, c.tc, c.words), slices, scratch, s,
                            [=](const TileGeom &g, uint64_t *dst, unsigned ns, bool final) {
                                return launch_words<MatmulPlainTerm, MatmulPlainTiles>(mods, pl, a, dst, g, ns, c, final, s);
                            });
    }

    unsigned matmul_scalars_row_tile(bool narrow)
    {
        return narrow ? kMatmulScalarsNarrowTile : kMatmulScalarsTile;
    }
    unsigned matmul_scalars_narrow_flush()
    {
        return kNarrowFlush;
    }
    size_t matmul_scalars_threads(unsigned size, size_t rows, size_t cols, unsigned n_log, unsigned K, bool narrow, unsigned row_tile)
    {
        const unsigned R = row_tile ? row_tile : matmul_scalars_row_tile(narrow);
        if (!MatmulScalarsTiles::with(R, 1, [](auto) {}) || rows * cols > 0xffffffffu)
            return 0;
        return tiled_threads(size, rows, cols, n_log, K, R, 1, 2);
    }
    hipError_t k_matmul_scalars(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                size_t r_stride, unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols,
                                bool a_transposed, bool r_transposed, unsigned slices, uint64_t *scratch, unsigned row_tile, hipStream_t s)
    {
        return scalars_reduce<MatmulScalarsTiles>(mods, weights, narrow, a, a_stride, r, r_stride, size, n_log, K, rows, inner, cols, a_transposed,
                                                  r_transposed, slices, scratch, row_tile ? row_tile : matmul_scalars_row_tile(narrow), s);
    }

    const char *conv2d_shape_error(const Conv2dShape &c, size_t &oh, size_t &ow)
    {
        const uint64_t lim = uint64_t(1) << 32;
        if (!c.in_channels || !c.height || !c.width || !c.out_channels || !c.kernel_h || !c.kernel_w || !c.stride_h || !c.stride_w)
            return "an extent or stride of the convolution is 0";
        if (c.pad_h >= c.kernel_h || c.pad_w >= c.kernel_w)
            return "pad must be below the kernel: every output has a tap inside the image";
        // (from here on pad < kernel; every factor is checked before it is multiplied, so no product wraps)
        if (c.in_channels >= lim || c.height >= lim || c.width >= lim || c.out_channels >= lim || c.kernel_h >= lim || c.kernel_w >= lim)
            return "C * H * W, OC * OH * OW and OC * C * kh * kw must be below 2^32";
        if (c.height + 2 * c.pad_h < c.kernel_h || c.width + 2 * c.pad_w < c.kernel_w)
            return "the kernel is larger than the padded image";
        const uint64_t h = (c.height + 2 * c.pad_h - c.kernel_h) / c.stride_h + 1, w = (c.width + 2 * c.pad_w - c.kernel_w) / c.stride_w + 1;
        const uint64_t taps = c.kernel_h * c.kernel_w, image = c.height * c.width; // both below 2^64
        if (h >= lim || w >= lim || h * w >= lim || taps >= lim || image >= lim || c.in_channels * image >= lim || c.out_channels * h * w >= lim ||
            c.in_channels * taps >= lim || c.out_channels * c.in_channels * taps >= lim)
            return "C * H * W, OC * OH * OW and OC * C * kh * kw must be below 2^32";
        if (c.in_channels * taps * h * w >= lim)
            return "the result is too large for one launch: C * kh * kw * OH * OW must be below 2^32";
        oh = (size_t)h;
        ow = (size_t)w;
        return nullptr;
    }
    size_t conv2d_scalars_threads(unsigned size, const Conv2dShape &shape, unsigned n_log, unsigned K, bool narrow, unsigned row_tile)
    {
        size_t oh, ow;
        if (conv2d_shape_error(shape, oh, ow))
            return 0;
        return matmul_scalars_threads(size, shape.out_channels, oh * ow, n_log, K, narrow, row_tile);
    }
    // the tiled host path with rows = OC, inner = C * kh * kw, cols = OH * OW (a channel-last result is the transposed one), whose
    // launch completes the geometry with the input's strides and the shape
    hipError_t k_conv2d_scalars(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                size_t r_stride, unsigned size, unsigned n_log, unsigned K, const Conv2dShape &c, bool in_last, bool out_last,
                                unsigned slices, uint64_t *scratch, unsigned row_tile, unsigned hint, hipStream_t s)
    {
        size_t oh, ow;
        const unsigned R = row_tile ? row_tile : matmul_scalars_row_tile(narrow);
        if (conv2d_shape_error(c, oh, ow) || !MatmulScalarsTiles::with(R, 1, [](auto) {}) || hint > 2)
            return hipErrorInvalidValue;
        const bool nt = hint ? hint == 1 : kConvNonTemporal, uniform = n_log >= 7;
        const size_t words = (size_t)K << n_log, C = c.in_channels, H = c.height, W = c.width, inner = C * c.kernel_h * c.kernel_w, cols = oh * ow;
        return tiled_reduce(mods, 0, a_stride, false, r, r_stride, out_last, size, n_log, K, c.out_channels, inner, cols, R, 1,
                            tiled_threads(size, c.out_channels, cols, n_log, K, R, 1, 2), slices, scratch, s,
                            [=](const TileGeom &t, uint64_t *dst, unsigned ns, bool final) {
                                const ConvGeom g{ t,
                                                  in_last ? words : H * W * words,
                                                  in_last ? W * C * words : W * words,
                                                  in_last ? C * words : words,
                                                  oh > 1 ? (size_t)c.stride_h : 1,
                                                  ow > 1 ? (size_t)c.stride_w : 1,
                                                  (unsigned)H,
                                                  (unsigned)W,
                                                  (unsigned)ow,
                                                  (unsigned)c.kernel_h,
                                                  (unsigned)c.kernel_w,
                                                  (unsigned)c.pad_h,
                                                  (unsigned)c.pad_w };
                                hipError_t e = hipErrorInvalidValue;
                                MatmulScalarsTiles::with(R, 1, [&](auto tile) {
                                    constexpr unsigned kR = decltype(tile)::kRows;
                                    if (narrow)
                                        e = nt ? launch_tiled<ConvFamily<kR, true, true>>(mods, weights, a, dst, g, ns, uniform, final, s)
                                               : launch_tiled<ConvFamily<kR, true, false>>(mods, weights, a, dst, g, ns, uniform, final, s);
                                    else
                                        e = nt ? launch_tiled<ConvFamily<kR, false, true>>(mods, weights, a, dst, g, ns, uniform, final, s)
                                               : launch_tiled<ConvFamily<kR, false, false>>(mods, weights, a, dst, g, ns, uniform, final, s);
                                });
                                return e;
                            });
    }
} // namespace sealhip
