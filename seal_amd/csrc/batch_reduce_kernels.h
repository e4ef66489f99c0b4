// Kernels of the Evaluator's reductions over the items of a batch (evaluator.h: sum_items / dot_plain_device / dot_items): output
// item o is the sum of the `group` input items o * group .. o * group + group - 1, of their dyadic products with one NTT-form
// plaintext per item, or of the size-2 x size-2 tensor products of the items of two batches.
// HBM-streaming like plain_batch_kernels.h and with its conventions: one thread moves two adjacent words per operand with one
// 16-byte access, flat grids (one thread per output pair, no loop over the grid), one ModDesc per prime, and the non-temporal hint
// on every ciphertext and plaintext word - each is read once.
// Layouts: a ciphertext plane is [batch][K][N], so the items of a group are `group` consecutive [K][N] blocks of each plane; the
// plaintexts are [batch][K][N]; the result's planes are [batch / group][K][N].  The result must not be an operand.
// Accumulation is lazy (batch_reduce_kernels.hip: kSumFlush, kDotFlush): terms are added as plain integers and reduced once per
// flush interval.  Every result is the canonical residue of an exactly specified integer, so it does not depend on the schedule:
// the words are those of the reference's Evaluator::add_many over Evaluator::multiply_plain_inplace.
// Small results: one thread per output pair is too few threads when the result is small (N = 8192, K = 3, one output item: 24 k),
// so below a threshold the group is cut into `slices` runs of consecutive items, each reduced by workgroups of its own (the slow grid
// dimension) into scratch [slices][size][batch / group][K][N], and a second launch, of the sum over the slices, adds them.  No atomics:
// modular addition is exact and associative, the words do not depend on the cut.
// Item maps (evaluator.h: ItemMap; include/sealhip.h: Evaluator_SumItemsMapped ...): the same kernels with another walk.  Instead of
// the items o * group + t, term t of output item (row) o is the item a CSR list names: rows [off[o], off[o + 1]) of two lists of
// 32-bit item numbers in HBM, one per operand.  Rows may differ in length; the kernels read the lists (through the scalar cache
// from N = 128 on, where a wave never leaves its row) and nothing else changes - a modular sum does not depend on which items it is
// told to add, so the words are still those of add_many over the per-object forms on the named items.  A cut slices every row at
// the same positions, sized from the longest row; slices past the end of a shorter row store zeros.
#pragma once
#include "encrypt_kernels.h"

namespace sealhip
{
    // terms a lazy accumulator takes between two reductions (derived in batch_reduce_kernels.hip from "primes are below 2^60")
    unsigned batch_reduce_sum_flush();
    unsigned batch_reduce_dot_flush();
    unsigned batch_reduce_dot_items_flush(); // items, not products: the middle polynomial of a ciphertext product takes two per item
    // The library's rule: slices for a launch of `threads` threads (one per output pair: sum_items size * out_items * K * N / 2,
    // dot_plain_device and dot_items out_items * K * N / 2) that each add `group` terms.  1 = one launch, no scratch.
    unsigned batch_reduce_slices(size_t threads, size_t group);

    // Which operand items the terms of an output item are.  ItemWalk(group): the consecutive items o * group .. o * group + group - 1
    // of both operands.  Mapped (offsets != nullptr; device pointers, 32-bit words; rows = the output items): term t of row o,
    // offsets[o] <= t < offsets[o + 1], is item first[t] of the first operand and second[t] of the second (second == first: one
    // list).  Item numbers are NOT checked by the kernels: ItemMap_Create does that once.
    struct ItemWalk
    {
        size_t longest = 0; // terms of the longest row: what a cut slices
        size_t mean = 0;    // ceil(terms / rows): what the library's rule is asked with
        const uint32_t *offsets = nullptr, *first = nullptr, *second = nullptr;
        ItemWalk() = default;
        explicit ItemWalk(size_t group) : longest(group), mean(group) {}
        ItemWalk(size_t longest_row, size_t mean_row, const uint32_t *off, const uint32_t *f, const uint32_t *s)
            : longest(longest_row), mean(mean_row), offsets(off), first(f), second(s)
        {}
        bool mapped() const { return offsets != nullptr; }
    };
    // The rule for a walk: whether to cut, and into how many slices, is decided from the MEAN work per thread
    // (batch_reduce_slices(threads, walk.mean)); the slices are then sized from the longest row - per_slice = ceil(longest / slices) -
    // and the count is what that leaves non-empty.  Consecutive groups: mean = longest = group, the rule above.  A very skewed map
    // (one long row among short ones) is balanced by this cut and by nothing else.
    unsigned batch_reduce_slices(size_t threads, const ItemWalk &walk);
    // words of scratch a call with `slices` > 1 needs
    inline size_t batch_reduce_scratch_words(unsigned slices, unsigned size, size_t out_items, unsigned n_log, unsigned K)
    {
        return slices > 1 ? (((size_t)slices * size * out_items * K) << n_log) : 0;
    }

    // r[p][o][k][j] = sum_i a[p][o * group + i][k][j] mod q_k, p < size (written for consecutive groups here and below; with a mapped
    // walk the items are the named ones).  Plane p of the source is a + p * a_stride, of the result r + p * r_stride.  slices: 1, or
    // the cut described above with scratch of batch_reduce_scratch_words words (2 <= slices <= walk.longest).
    hipError_t k_sum_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, uint64_t *r, size_t r_stride, unsigned size, unsigned n_log,
                           unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices, uint64_t *scratch, hipStream_t s);
    // r[p][o][k][j] = sum_i a[p][o * group + i][k][j] * pl[o * group + i][k][j] mod q_k.  A thread keeps its two plaintext words in
    // registers over the planes (up to three at a time): the plaintexts cross HBM once for size <= 3.
    hipError_t k_dot_plain_items(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *pl, uint64_t *r, size_t r_stride,
                                 unsigned size, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices,
                                 uint64_t *scratch, hipStream_t s);
    // Ciphertext x ciphertext, both of size 2 and in NTT form: x, y = [2][batch][K][N] (planes x_stride / y_stride words apart),
    // r = [3][batch / group][K][N]:
    //   r[0][o] = sum_i x0 y0,  r[1][o] = sum_i (x0 y1 + x1 y0),  r[2][o] = sum_i x1 y1   over the items o * group + i, mod q_k
    // - the words of multiply (evaluator.cpp ckks_multiply / bgv_multiply, 2 x 2) per item and then add_many.  Each operand word
    // crosses HBM once: 4 plane-items read per item, no product is stored.  y == x (same pointer and stride, and one list of items
    // when the walk is mapped) is the sum of squares and reads 2.  slices, scratch: as above with size 3.
    hipError_t k_dot_items(const ModDesc *mods, const uint64_t *x, size_t x_stride, const uint64_t *y, size_t y_stride, uint64_t *r,
                           size_t r_stride, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk, unsigned slices,
                           uint64_t *scratch, hipStream_t s);

    // A sparse matrix of scalar weights times the items of a batch: k_dot_plain_items over a mapped walk with ONE value per prime (or
    // one for all primes) instead of [K][N] words per plaintext.  Term t of row o is item first[t] of a times weight second[t]:
    //   r[p][o][k][j] = sum_t const(w[second[t]])_k a[p][first[t]][k][j] mod q_k,  offsets[o] <= t < offsets[o + 1]
    // weights, wide (narrow false): [count][K] 64-bit words, word k of weight i at i * K + k - k_dot_scalars' scalars.  Narrow:
    // [count] signed 32-bit integers; weight w stands for the K words w mod q, so the result words are the wide form's on those.
    // The words are k_dot_plain_items' over the same walk with each weight expanded to [K][N].  Accumulation: the wide form's
    // sums are reduced once per batch_reduce_dot_flush() terms, the narrow form's (the biased weight and the two exact sums of
    // k_matmul_scalars) once per matmul_scalars_narrow_flush().  One thread = one pair of one plane (the planes are in the grid, as
    // for k_sum_items, so any size is one launch).  From N = 128 on offsets, lists and weights are scalar loads through the constant
    // cache: the weights must have been written by something earlier on the stream.  Weights are indexed in 64 bits: count * K has
    // no bound of its own (count is a map's second_batch, below 2^32).  The walk must be mapped - consecutive items are
    // k_dot_scalars'.  slices, scratch: the mapped cut as above with scratch of batch_reduce_scratch_words(slices, size, out_items,
    // ...) words; the library's rule is asked with size * out_items * K * N / 2 threads and the walk.  r must not be an operand.
    hipError_t k_dot_scalars_mapped(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                    size_t r_stride, unsigned size, unsigned n_log, unsigned K, size_t out_items, const ItemWalk &walk,
                                    unsigned slices, uint64_t *scratch, hipStream_t s);

    // Scalar weights: r[p][o][k][j] = sum_b a[p][b][k][j] * s[o][b][k] mod q_k for o < rows - a dense rows x batch matrix of scalar
    // plaintexts times the items of a batch.  scalars = [rows][batch][K] words: word k is the value every coefficient of prime k
    // holds in the NTT-form constant plaintext, so the words are those of k_dot_plain_items over the dense map with the scalars
    // expanded to [rows * batch][K][N].  A thread holds a tile of dot_scalars_row_tile() consecutive rows of one coefficient pair
    // and uses each loaded operand pair for all of them: the operand crosses HBM once per tile of rows.  From N = 128 on the
    // weights are read with scalar loads through the constant cache: they must have been written by something earlier on the
    // stream (a copy, a previous kernel).  rows * batch < 2^32.  slices, scratch: the cut of the batch as above, with scratch of
    // batch_reduce_scratch_words(slices, size, rows, ...) words; the library's rule is asked with dot_scalars_threads() threads
    // that each add `batch` terms.  row_tile: 0 = the library's, or one of the built ones (2, 4, 8: the rate tool's sweep).
    // It is k_matmul_scalars (below) at one column: the wide form with cols = 1, inner = batch and neither layout flag, run by the
    // same kernel.
    unsigned dot_scalars_row_tile();
    size_t dot_scalars_threads(unsigned size, size_t rows, unsigned n_log, unsigned K, unsigned row_tile = 0);
    hipError_t k_dot_scalars(const ModDesc *mods, const uint64_t *a, size_t a_stride, const uint64_t *scalars, uint64_t *r, size_t r_stride,
                             unsigned size, unsigned n_log, unsigned K, size_t rows, size_t batch, unsigned slices, uint64_t *scratch,
                             unsigned row_tile, hipStream_t s);

    // Ciphertext matrix x ciphertext matrix over the items of two batches: x = [2][rows * inner][K][N] with item (i, k) at
    // i * inner + k, y = [2][inner * cols][K][N] with item (k, j) at k * cols + j - or at j * inner + k when y_transposed -, both of
    // size 2 and in NTT form (planes x_stride / y_stride words apart), r = [3][rows * cols][K][N] with item (i, j) at i * cols + j:
    //   r[.][i][j] = sum_k x[i][k] (x) y[k][j],  the term being k_dot_items' (c0 += x0 y0, c1 += x0 y1 + x1 y0, c2 += x1 y1)
    // - word for word k_dot_items over the map whose row i * cols + j names the pairs (i * inner + k, k * cols + j).  A thread holds
    // a tile of TR consecutive output rows x TC consecutive output columns of one coefficient position of one prime, loads the TR
    // x-items and TC y-items of a k once and uses them for all TR TC outputs: 2 (TR + TC) plane-items read per TR TC terms, where
    // the map reads 4 per term.  Sums are plain 128-bit integers, reduced once per batch_reduce_dot_items_flush() values of k.
    // x == y (same pointer) is allowed; r must not be an operand.  Each of rows * inner, inner * cols and rows * cols < 2^32.
    // slices, scratch: the cut of the inner index as above, with scratch of batch_reduce_scratch_words(slices, 3, rows * cols, ...)
    // words; the library's rule is asked with matmul_items_threads() threads that each add `inner` terms.
    // tile: 0 = the library's, or matmul_items_tile_id(TR, TC) of a built one (1 x 1, 2 x 2, 2 x 4: the rate tool's sweep), to
    // which kMatmulItemsNonTemporal / kMatmulItemsCached may be added to give the operand loads the non-temporal hint or not (neither:
    // the library's choice).  matmul_items_threads is 0 for a tile that is not built and for a launch the flat grid refuses (rows of
    // the grid are numbered in 32 bits): k_matmul_items fails on both.
    constexpr unsigned matmul_items_tile_id(unsigned tile_rows, unsigned tile_cols)
    {
        return tile_rows << 8 | tile_cols;
    }
    constexpr unsigned kMatmulItemsNonTemporal = 1u << 16, kMatmulItemsCached = 2u << 16, kMatmulItemsHintMask = 3u << 16;
    void matmul_items_tile(unsigned &tile_rows, unsigned &tile_cols); // the library's
    size_t matmul_items_threads(size_t rows, size_t cols, unsigned n_log, unsigned K, unsigned tile = 0);
    hipError_t k_matmul_items(const ModDesc *mods, const uint64_t *x, size_t x_stride, const uint64_t *y, size_t y_stride, uint64_t *r,
                              size_t r_stride, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols, bool y_transposed,
                              unsigned slices, uint64_t *scratch, unsigned tile, hipStream_t s);

    // Plaintext matrix x ciphertext matrix over the items of a batch: pl = [rows * inner][K][N] NTT-form plaintexts with (i, k) at
    // i * inner + k, a = [size][inner * cols][K][N] in NTT form (planes a_stride words apart) with item (k, j) at k * cols + j - or at
    // j * inner + k when a_transposed -, r = [size][rows * cols][K][N] with item (i, j) at i * cols + j - or at j * rows + i when
    // r_transposed:
    //   r[p][i][j] = sum_k pl[i][k] a[p][k][j] mod q_k
    // - word for word k_dot_plain_items over the map whose row i * cols + j names item k * cols + j and plaintext i * inner + k.  A
    // thread holds a tile of TP consecutive output rows x TC consecutive output columns of one coefficient position of one prime and
    // one plane (the planes are in the grid, so any size is one launch), loads the TP plaintext words and TC ciphertext words of a
    // k once and uses them for all TP TC products: (TP + TC) / (TP TC) plane-items read per term and plane, where the map reads
    // (size + 1) / size.  Both layouts of a and of r are strides of the one kernel.  Sums are plain 128-bit integers, reduced once
    // per batch_reduce_dot_flush() values of k.  r must not be an operand.  Each of rows * inner, inner * cols, rows * cols < 2^32.
    // slices, scratch: the cut of the inner index as above, with scratch of batch_reduce_scratch_words(slices, size, rows * cols,
    // ...) words; the library's rule is asked with matmul_plain_items_threads() threads that each add `inner` terms.
    // tile: 0 = the library's, or matmul_items_tile_id(TP, TC) of a built one (1 x 1, 2 x 4, 4 x 4, 4 x 8: the rate tool's sweep),
    // to which kMatmulItemsNonTemporal / kMatmulItemsCached may be added as for k_matmul_items.  matmul_plain_items_threads is 0 for
    // a tile that is not built and for a launch the flat grid refuses: k_matmul_plain_items fails on both.
    void matmul_plain_items_tile(unsigned &tile_rows, unsigned &tile_cols); // the library's
    size_t matmul_plain_items_threads(unsigned size, size_t rows, size_t cols, unsigned n_log, unsigned K, unsigned tile = 0);
    hipError_t k_matmul_plain_items(const ModDesc *mods, const uint64_t *pl, const uint64_t *a, size_t a_stride, uint64_t *r, size_t r_stride,
                                    unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols, bool a_transposed,
                                    bool r_transposed, unsigned slices, uint64_t *scratch, unsigned tile, hipStream_t s);

    // Scalar weight matrix x ciphertext matrix over the items of a batch: k_matmul_plain_items with ONE value per prime (or one for
    // all primes) instead of [K][N] words per plaintext, and k_dot_scalars with a column index.  a, r, a_transposed, r_transposed,
    // slices and scratch are k_matmul_plain_items':
    //   r[p][i][j] = sum_k const(w[i][k]) a[p][k][j] mod q
    // weights, wide (narrow false): [rows * inner][K] 64-bit words, weight (i, k) at i * inner + k - k_dot_scalars' scalars, and with
    // cols = 1 and no flag its words.  Narrow: [rows * inner] signed 32-bit integers; weight w stands for the K words w mod q, so
    // the result words are the wide form's on those.  Its products are 32 x 64 bits - two multiplies each - and its sums are
    // reduced once per matmul_scalars_narrow_flush() values of k (the wide form's: batch_reduce_dot_flush()).  A thread holds a tile
    // of R consecutive output rows of one coefficient pair of one output column: the operand crosses HBM once per tile of rows.
    // From N = 128 on the weights are read with scalar loads through the constant cache: they must have been written by something
    // earlier on the stream.  Each of rows * inner, inner * cols, rows * cols < 2^32; r must not be an operand.
    // The library's rule is asked with matmul_scalars_threads() threads that each add `inner` terms; it is 0 for a tile that is not
    // built and for a launch the flat grid refuses: k_matmul_scalars fails on both.  row_tile: 0 = the library's for the form, or
    // one of the built ones (4, 8: the rate tool's sweep).
    unsigned matmul_scalars_row_tile(bool narrow);
    unsigned matmul_scalars_narrow_flush();
    size_t matmul_scalars_threads(unsigned size, size_t rows, size_t cols, unsigned n_log, unsigned K, bool narrow, unsigned row_tile = 0);
    hipError_t k_matmul_scalars(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                size_t r_stride, unsigned size, unsigned n_log, unsigned K, size_t rows, size_t inner, size_t cols,
                                bool a_transposed, bool r_transposed, unsigned slices, uint64_t *scratch, unsigned row_tile, hipStream_t s);

    // 2-D convolution of scalar weights over a grid of items: k_matmul_scalars with rows = the output channels, cols = the output
    // positions OH * OW and inner = C * kh * kw, whose operand of term t = (c * kh + dy) * kw + dx at output position (y', x') is
    // not item (t, j) of a dense matrix but input item (c, y' sh + dy - ph, x' sw + dx - pw) - no gathered batch exists:
    //   r[p][o][y'][x'] = sum_{c, dy, dx} const(w[o][(c * kh + dy) * kw + dx]) a[p][c][y' sh + dy - ph][x' sw + dx - pw] mod q
    // over the taps inside the image; the others are skipped, not read.  OH = (H + 2 ph - kh) / sh + 1, OW likewise.
    // a = [size][C * H * W][K][N], item (c, y, x) at (c * H + y) * W + x - or at (y * W + x) * C + c when in_last -, r = [size][OC *
    // OH * OW][K][N], item (o, y', x') at (o * OH + y') * OW + x' - or at (y' * OW + x') * OC + o when out_last: strides, as the
    // layouts of k_matmul_scalars.  weights, narrow, the tile of R output channels per thread, the flush intervals (which count
    // executed taps) and "written by something earlier on the stream" are k_matmul_scalars'.  From N = 128 on the output position
    // is wave-uniform like the column there, and with it the in-image range of dy and dx.
    // conv2d_shape_error: nullptr, or what is wrong with a shape - an extent or stride of 0, pad >= kernel (so every output has a
    // tap), H + 2 ph < kh (or the width), or one of C H W, OC OH OW, OC inner, inner OH OW >= 2^32 (the last is the skeleton's bound
    // on the terms of a launch); oh and ow are set when it is nullptr.
    // slices, scratch: a cut of the flat term index t as above, with scratch of batch_reduce_scratch_words(slices, size, OC * OH *
    // OW, ...) words; a slice without a live term for some output stores zeros there.  The library's rule is asked with
    // conv2d_scalars_threads() threads that each add `inner` terms; it is 0 for a tile that is not built, a shape that is refused
    // and a launch the flat grid refuses: k_conv2d_scalars fails on all three.  row_tile: 0 or 4, 8 as k_matmul_scalars.
    // hint: the operand loads carry the non-temporal hint (1) or not (2), 0 = the library's choice: unlike the product's operand an
    // input item is read by up to ceil(kh / sh) ceil(kw / sw) neighbouring outputs, times ceil(OC / R) channel tiles.
    struct Conv2dShape
    {
        uint64_t in_channels, height, width, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w;
    };
    const char *conv2d_shape_error(const Conv2dShape &shape, size_t &oh, size_t &ow);
    size_t conv2d_scalars_threads(unsigned size, const Conv2dShape &shape, unsigned n_log, unsigned K, bool narrow, unsigned row_tile = 0);
    hipError_t k_conv2d_scalars(const ModDesc *mods, const void *weights, bool narrow, const uint64_t *a, size_t a_stride, uint64_t *r,
                                size_t r_stride, unsigned size, unsigned n_log, unsigned K, const Conv2dShape &shape, bool in_last,
                                bool out_last, unsigned slices, uint64_t *scratch, unsigned row_tile, unsigned hint, hipStream_t s);
} // namespace sealhip
