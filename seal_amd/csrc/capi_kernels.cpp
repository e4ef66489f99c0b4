// extern "C" layer, part 4: the per-kernel seam (NTT, dyadic products, RNS stages on raw device buffers; include/sealhip.h)
#include "capi_common.h"
#include "batch_reduce_kernels.h"
#include <memory>

namespace
{
    // The prologue of the raw seams of the batch reductions (shl_reduce_items, shl_dot_items, shl_reduce_mapped): level and cut are
    // checked - slices == 0 asks for the library's rule over grid_planes * (one result plane) / 2 threads and this walk -, *slices_used
    // is set, a call without a result is the query and ends there; otherwise launch(context, level, words per item, slices) runs
    template <class Launch>
    SHL_HRESULT raw_reduce(void *context, uint64_t chain_index, const char *shape_error, uint64_t grid_planes, uint64_t out_items,
                           const ItemWalk &walk, uint64_t slices, uint64_t *slices_used, const uint64_t *r, bool operands,
                           const uint64_t *scratch, Launch launch)
    {
        IfNullRet(context, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        auto l = c->level_by_chain_index(chain_index);
        if (!l)
            throw std::out_of_range("chain_index");
        if (shape_error)
            throw std::invalid_argument(shape_error);
        const size_t words = (size_t)l->K * c->n();
        if (!slices)
            slices = batch_reduce_slices(grid_planes * out_items * words / 2, walk);
        if (slices > walk.longest || slices > 64)
            throw std::invalid_argument("1 <= slices <= min(group or longest row, 64)");
        if (slices_used)
            *slices_used = slices;
        if (!r) // a query: the slices the library would use, hence the scratch to pass
            return SHL_S_OK;
        IfNullRet(operands, SHL_E_POINTER);
        if (slices > 1 && !scratch)
            throw std::invalid_argument("scratch is null");
        launch(c, l, words, (unsigned)slices);
        SHL_CATCH
    }
    // consecutive groups: the shape is checked here
    template <class Launch>
    SHL_HRESULT raw_reduce(void *context, uint64_t chain_index, bool size_ok, const char *shape, uint64_t grid_planes, uint64_t batch,
                           uint64_t group, uint64_t slices, uint64_t *slices_used, const uint64_t *r, bool operands, const uint64_t *scratch,
                           Launch launch)
    {
        const bool bad = !group || batch % group || !size_ok;
        const size_t out_items = bad ? 0 : batch / group;
        const ItemWalk walk(group);
        return raw_reduce(context, chain_index, bad ? shape : nullptr, grid_planes, out_items, walk, slices, slices_used, r, operands, scratch,
                          [&](Context *c, const Level *l, size_t words, unsigned cut) { launch(c, l, out_items, words, walk, cut); });
    }
    // The prologue of the raw seams of the tiled products (shl_dot_scalars_tile, shl_matmul_items_tile, shl_matmul_plain_items_tile,
    // shl_matmul_scalars_tile), rows x inner times inner x cols with `planes` result planes: the level, then `error` (the entry's
    // own checks, NULL = passed), then the shape - shape_error when a dimension is 0 or beyond 32 bits, a product of two is, or
    // threads(n_log, K) is 0: a tile that is not built or a launch the flat grid refuses.  slices == 0 asks for the library's rule
    // over those threads; *slices_used is set, a call without a result is the query and ends there; otherwise the pool gives the
    // scratch and launch(context, level, n_log, words per item, slices, scratch, stream) runs inside a StreamScope.
    // Two differences between the entries are kept as they were.  shl_dot_scalars_tile checks its shape and tile itself, under its
    // own message (shape_error NULL), and leaves a grid that does not fit to the launch.  Only shl_matmul_scalars_tile reports
    // (and allocates for) the slices the cut leaves non-empty (normalise); the others report the slices asked for.
    template <class Threads, class Launch>
    SHL_HRESULT raw_tiled(void *context, uint64_t chain_index, const char *error, const char *shape_error, const char *slices_error,
                          uint64_t planes, uint64_t rows, uint64_t inner, uint64_t cols, uint64_t slices, bool normalise, uint64_t *slices_used,
                          const uint64_t *r, const void *x, const void *y, void *stream, Threads threads, Launch launch)
    {
        IfNullRet(context, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        auto l = c->level_by_chain_index(chain_index);
        if (!l)
            throw std::out_of_range("chain_index");
        if (error)
            throw std::invalid_argument(error);
        const unsigned n_log = (unsigned)c->log_n();
        const size_t count = threads(n_log, l->K);
        if (shape_error && (!rows || !inner || !cols || (rows >> 32) || (inner >> 32) || (cols >> 32) || ((rows * inner) >> 32) ||
                            ((inner * cols) >> 32) || ((rows * cols) >> 32) || !count))
            throw std::invalid_argument(shape_error);
        if (!slices)
            slices = batch_reduce_slices(count, inner);
        if (slices > inner || slices > 64)
            throw std::invalid_argument(slices_error);
        if (normalise)
            slices = (inner + (inner + slices - 1) / slices - 1) / ((inner + slices - 1) / slices); // those the cut leaves non-empty
        if (slices_used)
            *slices_used = slices;
        if (!r) // a query: the slices the library would use
            return SHL_S_OK;
        IfNullRet(x, SHL_E_POINTER);
        IfNullRet(y, SHL_E_POINTER);
        hipStream_t s = (hipStream_t)stream;
        StreamScope scope(s);
        std::unique_ptr<Scratch> scratch;
        if (slices > 1)
            scratch.reset(new Scratch(batch_reduce_scratch_words((unsigned)slices, (unsigned)planes, rows * cols, n_log, l->K)));
        launch(c, l, n_log, (size_t)l->K * c->n(), (unsigned)slices, scratch ? scratch->p : nullptr, s);
        SHL_CATCH
    }
    // What the entries without a stream argument add to their _tile form, which ran on the NULL stream: the call returns when the
    // work is done.  A refusal or a query (r == NULL) has queued nothing and is handed back as it is.
    SHL_HRESULT then_synchronise(SHL_HRESULT hr, const uint64_t *r, const char *what)
    {
        if (hr != SHL_S_OK || !r)
            return hr;
        SHL_TRY
        hip_ok(hipStreamSynchronize(nullptr), what);
        SHL_CATCH
    }
    constexpr const char *kMatmulShape = "1 <= rows, inner, cols; rows * inner, inner * cols, rows * cols < 2^32; a built tile";
    constexpr const char *kMatmulSlices = "1 <= slices <= min(inner, 64)";
} // namespace

extern "C"
{
    // ------------------------------------------------------------------ per-kernel seam
    SHL_FUNC shl_ntt_forward(void *context, uint64_t *data, uint64_t polys, uint64_t comps, uint64_t first_prime, int lazy, void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(data, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        if (first_prime + comps > c->pool_primes().size())
            throw std::out_of_range("first_prime + comps");
        const NttBatch b = plain_batch(data, (size_t)comps * c->n(), (unsigned)comps, (unsigned)polys, (unsigned)first_prime);
        hip_ok(ntt_forward(c->ntt_tables(), b, lazy, (hipStream_t)stream), "ntt_forward");
        SHL_CATCH
    }
    SHL_FUNC shl_ntt_inverse(void *context, uint64_t *data, uint64_t polys, uint64_t comps, uint64_t first_prime, int lazy, void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(data, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        if (first_prime + comps > c->pool_primes().size())
            throw std::out_of_range("first_prime + comps");
        const NttBatch b = plain_batch(data, (size_t)comps * c->n(), (unsigned)comps, (unsigned)polys, (unsigned)first_prime);
        hip_ok(ntt_inverse(c->ntt_tables(), b, lazy, (hipStream_t)stream), "ntt_inverse");
        SHL_CATCH
    }
    SHL_FUNC shl_dyadic_product(
        void *context, const uint64_t *a, const uint64_t *b, uint64_t *r, uint64_t polys, uint64_t comps, uint64_t first_prime,
        void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(a, SHL_E_POINTER);
        IfNullRet(b, SHL_E_POINTER);
        IfNullRet(r, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        if (first_prime + comps > c->pool_primes().size())
            throw std::out_of_range("first_prime + comps");
        hip_ok(k_dyadic(c->dev_mods(), a, b, r, (unsigned)c->log_n(), (unsigned)comps, (unsigned)first_prime, polys, (hipStream_t)stream), "dyadic");
        SHL_CATCH
    }
    SHL_FUNC shl_reduce_items(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *plain, uint64_t *r, uint64_t size,
                              uint64_t batch, uint64_t group, uint64_t slices, uint64_t *scratch, uint64_t *slices_used, void *stream)
    {
        return raw_reduce(context, chain_index, size && size <= 16, "group must divide batch; 1 <= size <= 16", plain ? 1 : size, batch, group,
                          slices, slices_used, r, a, scratch, [&](Context *c, const Level *l, size_t out_items, size_t words, const ItemWalk &walk, unsigned cut) {
                              const unsigned n_log = (unsigned)c->log_n();
                              if (plain)
                                  hip_ok(k_dot_plain_items(c->dev_mods(), a, batch * words, plain, r, out_items * words, (unsigned)size, n_log, l->K,
                                                           out_items, walk, cut, scratch, (hipStream_t)stream),
                                         "dot_plain (items)");
                              else
                                  hip_ok(k_sum_items(c->dev_mods(), a, batch * words, r, out_items * words, (unsigned)size, n_log, l->K, out_items,
                                                     walk, cut, scratch, (hipStream_t)stream),
                                         "sum (items)");
                          });
    }
    SHL_FUNC shl_reduce_flush_intervals(uint64_t *sum_terms, uint64_t *dot_terms)
    {
        IfNullRet(sum_terms, SHL_E_POINTER);
        IfNullRet(dot_terms, SHL_E_POINTER);
        *sum_terms = batch_reduce_sum_flush();
        *dot_terms = batch_reduce_dot_flush();
        return SHL_S_OK;
    }
    SHL_FUNC shl_dot_items(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t batch,
                           uint64_t group, uint64_t slices, uint64_t *scratch, uint64_t *slices_used, void *stream)
    {
        return raw_reduce(context, chain_index, true, "group must divide batch", 1, batch, group, slices, slices_used, r, x && y, scratch,
                          [&](Context *c, const Level *l, size_t out_items, size_t words, const ItemWalk &walk, unsigned cut) {
                              hip_ok(k_dot_items(c->dev_mods(), x, batch * words, y, batch * words, r, out_items * words, (unsigned)c->log_n(), l->K,
                                                 out_items, walk, cut, scratch, (hipStream_t)stream),
                                     "dot (items)");
                          });
    }
    SHL_FUNC shl_dot_items_flush_interval(uint64_t *items)
    {
        IfNullRet(items, SHL_E_POINTER);
        *items = batch_reduce_dot_items_flush();
        return SHL_S_OK;
    }
    SHL_FUNC shl_reduce_mapped(void *context, uint64_t chain_index, int kind, const uint64_t *a, uint64_t a_batch, const uint64_t *b,
                               uint64_t b_batch, uint64_t *r, uint64_t size, void *item_map, uint64_t slices, uint64_t *scratch,
                               uint64_t *slices_used, void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(item_map, SHL_E_POINTER);
        const ItemMap *m = as<ItemMap>(item_map);
        const bool two = kind != 0; // a second operand: the plaintexts, or y
        const bool bad = kind < 0 || kind > 2 || !size || size > 16 || a_batch != m->first_batch() || (two && b_batch != m->second_batch());
        const size_t rows = m->rows();
        const ItemWalk walk = m->walk();
        return raw_reduce(context, chain_index, bad ? "kind 0 .. 2; 1 <= size <= 16; the batches are the map's" : nullptr, kind == 0 ? size : 1, rows, walk, slices, slices_used, r, a && (b || !two), scratch,
                          [&](Context *c, const Level *l, size_t words, unsigned cut) {
                              const unsigned n_log = (unsigned)c->log_n();
                              hipStream_t s = (hipStream_t)stream;
                              if (kind == 0)
                                  hip_ok(k_sum_items(c->dev_mods(), a, a_batch * words, r, rows * words, (unsigned)size, n_log, l->K, rows, walk, cut,
                                                     scratch, s),
                                         "sum (mapped)");
                              else if (kind == 1)
                                  hip_ok(k_dot_plain_items(c->dev_mods(), a, a_batch * words, b, r, rows * words, (unsigned)size, n_log, l->K, rows,
                                                           walk, cut, scratch, s),
                                         "dot_plain (mapped)");
                              else
                                  hip_ok(k_dot_items(c->dev_mods(), a, a_batch * words, b, b_batch * words, r, rows * words, n_log, l->K, rows, walk,
                                                     cut, scratch, s),
                                         "dot (mapped)");
                          });
    }
    // k_dot_scalars_mapped on raw words, with shl_reduce_mapped's conventions: weights [weight_count][K] 64-bit words or, narrow,
    // [weight_count] signed 32-bit integers, a [size][a_batch][K][N], r [size][rows][K][N]; slices == 0: the library's rule over
    // size * rows * K * N / 2 threads; r == NULL: the query; scratch [slices][size][rows][K][N] words from the caller when cut
    SHL_FUNC shl_dot_scalars_mapped(void *context, uint64_t chain_index, const void *weights, uint64_t weight_count, int narrow, const uint64_t *a,
                                    uint64_t a_batch, uint64_t *r, uint64_t size, void *item_map, uint64_t slices, uint64_t *scratch,
                                    uint64_t *slices_used, void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(item_map, SHL_E_POINTER);
        const ItemMap *m = as<ItemMap>(item_map);
        const bool bad = !size || size > 16 || a_batch != m->first_batch() || weight_count != m->second_batch();
        const size_t rows = m->rows();
        const ItemWalk walk = m->walk();
        return raw_reduce(context, chain_index, bad ? "1 <= size <= 16; the batch and the weight count are the map's" : nullptr, size, rows, walk, slices,
                          slices_used, r, a && weights, scratch, [&](Context *c, const Level *l, size_t words, unsigned cut) {
                              hip_ok(k_dot_scalars_mapped(c->dev_mods(), weights, narrow != 0, a, a_batch * words, r, rows * words, (unsigned)size,
                                                          (unsigned)c->log_n(), l->K, rows, walk, cut, scratch, (hipStream_t)stream),
                                     "dot_scalars (mapped)");
                          });
    }
    SHL_FUNC shl_dot_scalars_mapped_info(uint64_t *flush, uint64_t *narrow_flush)
    {
        IfNullRet(flush, SHL_E_POINTER);
        IfNullRet(narrow_flush, SHL_E_POINTER);
        *flush = batch_reduce_dot_flush();
        *narrow_flush = matmul_scalars_narrow_flush();
        return SHL_S_OK;
    }
    // k_dot_scalars on raw words: a [size][batch][K][N], scalars [rows][batch][K], r [size][rows][K][N]; slices == 0: the library's
    // rule; r == NULL: the query.  Scratch comes from the pool; the NULL stream, and the call returns when the work is done.
    // row_tile: 0 = the library's (what shl_dot_scalars runs); 2, 4, 8 are built for tools/dot_scalars_rate.py
    SHL_FUNC shl_dot_scalars_tile(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *scalars, uint64_t *r, uint64_t size,
                                  uint64_t rows, uint64_t batch, uint64_t slices, uint64_t *slices_used, uint64_t row_tile, void *stream)
    {
        const bool bad = !size || size > 16 || !rows || !batch || (rows >> 32) || (batch >> 32) || ((rows * batch) >> 32) ||
                         (row_tile && row_tile != 2 && row_tile != 4 && row_tile != 8);
        return raw_tiled(
            context, chain_index, bad ? "1 <= size <= 16; 1 <= rows, batch; rows * batch < 2^32; row_tile 0, 2, 4 or 8" : nullptr, nullptr,
            "1 <= slices <= min(batch, 64)", size, rows, batch, 1, slices, false, slices_used, r, a, scalars, stream,
            [&](unsigned n_log, unsigned K) { return dot_scalars_threads((unsigned)size, rows, n_log, K, (unsigned)row_tile); },
            [&](Context *c, const Level *l, unsigned n_log, size_t words, unsigned cut, uint64_t *scratch, hipStream_t s) {
                hip_ok(k_dot_scalars(c->dev_mods(), a, batch * words, scalars, r, rows * words, (unsigned)size, n_log, l->K, rows, batch, cut, scratch,
                                     (unsigned)row_tile, s),
                       "dot_scalars");
            });
    }
    SHL_FUNC shl_dot_scalars(void *context, uint64_t chain_index, const uint64_t *a, const uint64_t *scalars, uint64_t *r, uint64_t size,
                             uint64_t rows, uint64_t batch, uint64_t slices, uint64_t *slices_used)
    {
        return then_synchronise(
            shl_dot_scalars_tile(context, chain_index, a, scalars, r, size, rows, batch, slices, slices_used, 0, nullptr),
            r, "dot_scalars sync");
    }
    SHL_FUNC shl_dot_scalars_info(uint64_t *row_tile, uint64_t *flush)
    {
        IfNullRet(row_tile, SHL_E_POINTER);
        IfNullRet(flush, SHL_E_POINTER);
        *row_tile = dot_scalars_row_tile();
        *flush = batch_reduce_dot_flush();
        return SHL_S_OK;
    }
    // k_matmul_items on raw words: x [2][rows * inner][K][N], y [2][inner * cols][K][N] ([cols][inner] items with y_transposed),
    // r [3][rows * cols][K][N]; slices == 0: the library's rule; r == NULL: the query.  Scratch comes from the pool.
    // tile: 0 = the library's (what shl_matmul_items runs); otherwise tile_rows << 8 | tile_cols of a built tile, plus 1 << 16 /
    // 2 << 16 for operand loads with / without the non-temporal hint - the sweep of tools/matmul_items_rate.py
    SHL_FUNC shl_matmul_items_tile(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t rows,
                                   uint64_t inner, uint64_t cols, int y_transposed, uint64_t slices, uint64_t *slices_used, uint64_t tile,
                                   void *stream)
    {
        return raw_tiled(
            context, chain_index, nullptr, kMatmulShape, kMatmulSlices, 3, rows, inner, cols, slices, false, slices_used, r, x, y, stream,
            [&](unsigned n_log, unsigned K) { return (tile >> 32) ? 0 : matmul_items_threads(rows, cols, n_log, K, (unsigned)tile); },
            [&](Context *c, const Level *l, unsigned n_log, size_t words, unsigned cut, uint64_t *scratch, hipStream_t s) {
                hip_ok(k_matmul_items(c->dev_mods(), x, rows * inner * words, y, inner * cols * words, r, rows * cols * words, n_log, l->K, rows,
                                      inner, cols, y_transposed != 0, cut, scratch, (unsigned)tile, s),
                       "matmul_items");
            });
    }
    SHL_FUNC shl_matmul_items(void *context, uint64_t chain_index, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t rows, uint64_t inner,
                              uint64_t cols, int y_transposed, uint64_t slices, uint64_t *slices_used)
    {
        return then_synchronise(
            shl_matmul_items_tile(context, chain_index, x, y, r, rows, inner, cols, y_transposed, slices, slices_used, 0, nullptr),
            r, "matmul_items sync");
    }
    SHL_FUNC shl_matmul_items_info(uint64_t *tile_rows, uint64_t *tile_cols, uint64_t *flush)
    {
        IfNullRet(tile_rows, SHL_E_POINTER);
        IfNullRet(tile_cols, SHL_E_POINTER);
        IfNullRet(flush, SHL_E_POINTER);
        unsigned tr, tc;
        matmul_items_tile(tr, tc);
        *tile_rows = tr;
        *tile_cols = tc;
        *flush = batch_reduce_dot_items_flush();
        return SHL_S_OK;
    }
    // k_matmul_plain_items on raw words: pl [rows * inner][K][N], a [size][inner * cols][K][N] ([cols][inner] items with flags bit 0),
    // r [size][rows * cols][K][N] ([cols][rows] items with flags bit 1); slices == 0: the library's rule; r == NULL: the query.
    // Scratch comes from the pool.  tile: 0 = the library's (what shl_matmul_plain_items runs); otherwise tile_rows << 8 | tile_cols
    // of a built tile, plus 1 << 16 / 2 << 16 for operand loads with / without the non-temporal hint - the sweep of
    // tools/matmul_plain_items_rate.py
    SHL_FUNC shl_matmul_plain_items_tile(void *context, uint64_t chain_index, const uint64_t *pl, const uint64_t *a, uint64_t *r, uint64_t size,
                                         uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used,
                                         uint64_t tile, void *stream)
    {
        const bool bad = !size || size > 16 || (flags & ~uint64_t(3));
        return raw_tiled(
            context, chain_index, bad ? "1 <= size <= 16; flags 0 .. 3" : nullptr, kMatmulShape, kMatmulSlices, size, rows, inner, cols, slices,
            false, slices_used, r, pl, a, stream,
            [&](unsigned n_log, unsigned K) {
                return (tile >> 32) ? 0 : matmul_plain_items_threads((unsigned)size, rows, cols, n_log, K, (unsigned)tile);
            },
            [&](Context *c, const Level *l, unsigned n_log, size_t words, unsigned cut, uint64_t *scratch, hipStream_t s) {
                hip_ok(k_matmul_plain_items(c->dev_mods(), pl, a, inner * cols * words, r, rows * cols * words, (unsigned)size, n_log, l->K, rows,
                                            inner, cols, (flags & 1) != 0, (flags & 2) != 0, cut, scratch, (unsigned)tile, s),
                       "matmul_plain_items");
            });
    }
    SHL_FUNC shl_matmul_plain_items(void *context, uint64_t chain_index, const uint64_t *pl, const uint64_t *a, uint64_t *r, uint64_t size,
                                    uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used)
    {
        return then_synchronise(
            shl_matmul_plain_items_tile(context, chain_index, pl, a, r, size, rows, inner, cols, flags, slices, slices_used, 0, nullptr),
            r, "matmul_plain_items sync");
    }
    SHL_FUNC shl_matmul_plain_items_info(uint64_t *tile_rows, uint64_t *tile_cols, uint64_t *flush)
    {
        IfNullRet(tile_rows, SHL_E_POINTER);
        IfNullRet(tile_cols, SHL_E_POINTER);
        IfNullRet(flush, SHL_E_POINTER);
        unsigned tp, tc;
        matmul_plain_items_tile(tp, tc);
        *tile_rows = tp;
        *tile_cols = tc;
        *flush = batch_reduce_dot_flush();
        return SHL_S_OK;
    }
    // k_matmul_scalars on raw words: weights [rows * inner][K] 64-bit words or, flags bit 2, [rows * inner] signed 32-bit integers,
    // a [size][inner * cols][K][N] ([cols][inner] items with flags bit 0), r [size][rows * cols][K][N] ([cols][rows] items with flags
    // bit 1); slices == 0: the library's rule; r == NULL: the query.  Scratch comes from the pool.  row_tile: 0 = the library's for
    // the form (what shl_matmul_scalars runs); 4 and 8 are built - the sweep of tools/matmul_scalars_rate.py
    SHL_FUNC shl_matmul_scalars_tile(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                     uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used,
                                     uint64_t row_tile, void *stream)
    {
        const bool bad = !size || size > 16 || (flags & ~uint64_t(7)), narrow = (flags & 4) != 0;
        return raw_tiled(
            context, chain_index, bad ? "1 <= size <= 16; flags 0 .. 7" : nullptr,
            "1 <= rows, inner, cols; rows * inner, inner * cols, rows * cols < 2^32; a built row tile", kMatmulSlices, size, rows, inner, cols,
            slices, true, slices_used, r, weights, a, stream,
            [&](unsigned n_log, unsigned K) {
                return (row_tile >> 32) ? 0 : matmul_scalars_threads((unsigned)size, rows, cols, n_log, K, narrow, (unsigned)row_tile);
            },
            [&](Context *c, const Level *l, unsigned n_log, size_t words, unsigned cut, uint64_t *scratch, hipStream_t s) {
                hip_ok(k_matmul_scalars(c->dev_mods(), weights, narrow, a, inner * cols * words, r, rows * cols * words, (unsigned)size, n_log, l->K,
                                        rows, inner, cols, (flags & 1) != 0, (flags & 2) != 0, cut, scratch, (unsigned)row_tile, s),
                       "matmul_scalars");
            });
    }
    SHL_FUNC shl_matmul_scalars(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags, uint64_t slices, uint64_t *slices_used)
    {
        return then_synchronise(
            shl_matmul_scalars_tile(context, chain_index, weights, a, r, size, rows, inner, cols, flags, slices, slices_used, 0, nullptr),
            r, "matmul_scalars sync");
    }
    SHL_FUNC shl_matmul_scalars_info(uint64_t *row_tile, uint64_t *narrow_row_tile, uint64_t *flush, uint64_t *narrow_flush)
    {
        IfNullRet(row_tile, SHL_E_POINTER);
        IfNullRet(narrow_row_tile, SHL_E_POINTER);
        IfNullRet(flush, SHL_E_POINTER);
        IfNullRet(narrow_flush, SHL_E_POINTER);
        *row_tile = matmul_scalars_row_tile(false);
        *narrow_row_tile = matmul_scalars_row_tile(true);
        *flush = batch_reduce_dot_flush();
        *narrow_flush = matmul_scalars_narrow_flush();
        return SHL_S_OK;
    }
    // k_conv2d_scalars on raw words: weights [OC * inner][K] 64-bit words or, flags bit 2, [OC * inner] signed 32-bit integers with
    // inner = C * kh * kw, a [size][C * H * W][K][N] (channel-last items with flags bit 0), r [size][OC * OH * OW][K][N] (channel-last
    // items with flags bit 1); slices == 0: the library's rule; r == NULL: the query.  Scratch comes from the pool.  row_tile: as
    // shl_matmul_scalars_tile; hint: 0 = the library's choice, 1 / 2 = operand loads with / without the non-temporal hint - the
    // sweep of tools/conv2d_scalars_rate.py
    SHL_FUNC shl_conv2d_scalars_tile(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                     const SHL_CONV2D *shape, uint64_t flags, uint64_t slices, uint64_t *slices_used, uint64_t row_tile,
                                     uint64_t hint, void *stream)
    {
        const bool narrow = (flags & 4) != 0;
        Conv2dShape c{};
        if (shape)
            c = Conv2dShape{ shape->in_channels, shape->height,   shape->width,    shape->out_channels, shape->kernel_h,
                             shape->kernel_w,    shape->stride_h, shape->stride_w, shape->pad_h,        shape->pad_w };
        size_t oh = 0, ow = 0;
        const char *error = !size || size > 16 || (flags & ~uint64_t(7)) || hint > 2 ? "1 <= size <= 16; flags 0 .. 7; hint 0 .. 2"
                            : !shape                                                ? "shape is null"
                                                                                    : conv2d_shape_error(c, oh, ow);
        const uint64_t inner = error ? 0 : c.in_channels * c.kernel_h * c.kernel_w;
        return raw_tiled(
            context, chain_index, error, "a result too large for one launch; a built row tile", "1 <= slices <= min(C * kh * kw, 64)", size,
            c.out_channels, inner, oh * ow, slices, true, slices_used, r, weights, a, stream,
            [&](unsigned n_log, unsigned K) {
                return (row_tile >> 32) ? 0 : conv2d_scalars_threads((unsigned)size, c, n_log, K, narrow, (unsigned)row_tile);
            },
            [&](Context *ctx, const Level *l, unsigned n_log, size_t words, unsigned cut, uint64_t *scratch, hipStream_t s) {
                hip_ok(k_conv2d_scalars(ctx->dev_mods(), weights, narrow, a, c.in_channels * c.height * c.width * words, r,
                                        c.out_channels * oh * ow * words, (unsigned)size, n_log, l->K, c, (flags & 1) != 0, (flags & 2) != 0, cut,
                                        scratch, (unsigned)row_tile, (unsigned)hint, s),
                       "conv2d_scalars");
            });
    }
    SHL_FUNC shl_conv2d_scalars(void *context, uint64_t chain_index, const void *weights, const uint64_t *a, uint64_t *r, uint64_t size,
                                const SHL_CONV2D *shape, uint64_t flags, uint64_t slices, uint64_t *slices_used)
    {
        return then_synchronise(
            shl_conv2d_scalars_tile(context, chain_index, weights, a, r, size, shape, flags, slices, slices_used, 0, 0, nullptr),
            r, "conv2d_scalars sync");
    }
    SHL_FUNC shl_apply_galois(
        void *context, uint64_t chain_index, int ntt_form, uint32_t galois_elt, const uint64_t *in, uint64_t *out, uint64_t polys,
        void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(in, SHL_E_POINTER);
        IfNullRet(out, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        auto l = c->level_by_chain_index(chain_index);
        if (!l)
            throw std::out_of_range("chain_index");
        if (!(galois_elt & 1) || galois_elt >= 2 * c->n())
            throw std::invalid_argument("Galois element is not valid");
        if (in == out)
            throw std::invalid_argument("result cannot point to the same value as operand");
        PlaneGeom g{ (unsigned)c->log_n(), l->K, (unsigned)polys };
        hip_ok(k_apply_galois(c->dev_mods(), in, out, galois_elt, ntt_form, g, 1, (hipStream_t)stream), "apply_galois");
        SHL_CATCH
    }
    SHL_FUNC shl_rns_stage(void *context, uint64_t chain_index, int which, const uint64_t *in, uint64_t *out, uint64_t polys, void *stream)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(in, SHL_E_POINTER);
        IfNullRet(out, SHL_E_POINTER);
        SHL_TRY
        auto c = as<Context>(context);
        auto l = c->level_by_chain_index(chain_index);
        if (!l)
            throw std::out_of_range("chain_index");
        hipStream_t s = (hipStream_t)stream;
        const unsigned n_log = (unsigned)c->log_n();
        if (which >= 0 && which <= 3)
        {
            if (c->scheme() != Scheme::bfv)
                throw std::logic_error("BEHZ stages exist only for BFV contexts");
            hip_ok(k_behz_stage(c->dev_mods(), l->dev, which, in, out, n_log, polys, s), "behz stage");
        }
        else if (which == 4)
        {
            if (l->K < 2)
                throw std::invalid_argument("level has a single modulus");
            hip_ok(k_bfv_modswitch(c->dev_mods(), l->dev, in, out, n_log, polys, s), "divide_and_round_q_last");
        }
        else if (which == 5)
        {
            if (l->K < 2)
                throw std::invalid_argument("level has a single modulus");
            const unsigned K = l->K;
            const size_t N = c->n();
            Scratch copy(polys * K * N);
            hip_ok(hipMemcpyAsync(copy.p, in, polys * K * N * 8, hipMemcpyDeviceToDevice, s), "copy");
            uint64_t *last = copy.p + (size_t)(K - 1) * N;
            hip_ok(ntt_inverse(c->ntt_tables(), plain_batch(last, (size_t)K * N, 1, (unsigned)polys, K - 1), 0, s), "intt last");
            hip_ok(ntt_forward(c->ntt_tables(),
                               plain_batch(nullptr, (size_t)(K - 1) * N, K - 1, (unsigned)polys, 0)
                                   .rounded_src(last, (size_t)K * N, 1, 2, l->dev.half_q_last, l->dev.q_last, l->dev.round_fix)
                                   .epilogue(1, copy.p, (size_t)K * N, l->dev.inv_q_last_mod_q, out, nullptr, (size_t)(K - 1) * N),
                               1, s),
                   "ntt correction + combine");
            hip_ok(hipStreamSynchronize(s), "sync");
        }
        else if (which == 6 || which == 7)
        {
            // the fused kernels Evaluator::multiply / square run for BFV, on the caller's words
            if (c->scheme() != Scheme::bfv)
                throw std::logic_error("BEHZ stages exist only for BFV contexts");
            if (which == 6)
                hip_ok(k_behz_lift(c->dev_mods(), l->dev, in, out, n_log, polys, s), "behz lift");
            else if (polys)
            {
                // the kernel takes the base-q and the base-Bsk parts as two slabs of strides K N and |Bsk| N
                const size_t N = c->n(), q_words = (size_t)l->K * N, b_words = (size_t)l->dev.nBsk * N;
                Scratch dq(polys * q_words), dbsk(polys * b_words);
                for (uint64_t p = 0; p < polys; p++)
                {
                    const uint64_t *src = in + p * (q_words + b_words);
                    hip_ok(hipMemcpyAsync(dq.p + p * q_words, src, q_words * 8, hipMemcpyDeviceToDevice, s), "copy");
                    hip_ok(hipMemcpyAsync(dbsk.p + p * b_words, src + q_words, b_words * 8, hipMemcpyDeviceToDevice, s), "copy");
                }
                hip_ok(k_behz_floor_sk(c->dev_mods(), l->dev, dq.p, dbsk.p, out, n_log, polys, s), "behz floor + sk");
                hip_ok(hipStreamSynchronize(s), "sync");
            }
        }
        else
            throw std::invalid_argument("unknown stage");
        SHL_CATCH
    }
    SHL_FUNC SealHip_SetStagedHostCopies(bool enabled)
    {
        set_staged_host_copies(enabled);
        return SHL_S_OK;
    }
    SHL_FUNC SealHip_ReleasePool(void)
    {
        SHL_TRY
        DevicePool::global().release_all();
        SHL_CATCH
    }
    SHL_FUNC SealHip_PoolStats(uint64_t *bytes_held, uint64_t *cross_stream_waits)
    {
        SHL_TRY
        if (bytes_held)
            *bytes_held = DevicePool::global().bytes_held();
        if (cross_stream_waits)
            *cross_stream_waits = DevicePool::global().cross_stream_waits();
        SHL_CATCH
    }
    SHL_FUNC SealHip_KsChunkStats(uint64_t *calls, uint64_t *chunks, uint64_t *scratch_bytes_max)
    {
        SHL_TRY
        uint64_t w = 0;
        ks_chunk_stats(calls, chunks, &w);
        if (scratch_bytes_max)
            *scratch_bytes_max = w * 8;
        SHL_CATCH
    }
    SHL_FUNC SealHip_XofStats(uint64_t *polynomials, uint64_t *replaced_words, uint64_t *host_walk_ns, uint64_t *total_ns)
    {
        SHL_TRY
        xof_stats(polynomials, replaced_words, host_walk_ns, total_ns);
        SHL_CATCH
    }
    SHL_FUNC SealHip_ProductStats(uint64_t *fused, uint64_t *formed, uint64_t *dropped)
    {
        SHL_TRY
        uint64_t f, p, d;
        lazy_product_stats(f, p, d);
        if (fused)
            *fused = f;
        if (formed)
            *formed = p;
        if (dropped)
            *dropped = d;
        SHL_CATCH
    }
    SHL_FUNC SealHip_GaloisStats(uint64_t *gathered, uint64_t *permuted)
    {
        SHL_TRY
        uint64_t g, p;
        galois_path_stats(g, p);
        if (gathered)
            *gathered = g;
        if (permuted)
            *permuted = p;
        SHL_CATCH
    }
    SHL_FUNC SealHip_GaloisSetStats(uint64_t *batched, uint64_t *looped, uint64_t *fused_launches)
    {
        SHL_TRY
        uint64_t b, l, f;
        galois_set_stats(b, l, f);
        if (batched)
            *batched = b;
        if (looped)
            *looped = l;
        if (fused_launches)
            *fused_launches = f;
        SHL_CATCH
    }
    SHL_FUNC SealHip_TailStats(uint64_t *folded, uint64_t *plain, uint64_t *dropped)
    {
        SHL_TRY
        uint64_t f, p, d;
        lazy_tail_stats(f, p, d);
        if (folded)
            *folded = f;
        if (plain)
            *plain = p;
        if (dropped)
            *dropped = d;
        SHL_CATCH
    }
    SHL_FUNC shl_device_count(int *count)
    {
        IfNullRet(count, SHL_E_POINTER);
        SHL_TRY
        *count = 0;
        if (hipGetDeviceCount(count) != hipSuccess)
            *count = 0;
        SHL_CATCH
    }
    SHL_FUNC shl_set_device(int device)
    {
        SHL_TRY
        hip_ok(hipSetDevice(device), "hipSetDevice");
        SHL_CATCH
    }
    SHL_FUNC shl_stream_create(bool non_blocking, void **hip_stream)
    {
        IfNullRet(hip_stream, SHL_E_POINTER);
        SHL_TRY
        hipStream_t s = nullptr;
        hip_ok(hipStreamCreateWithFlags(&s, non_blocking ? hipStreamNonBlocking : hipStreamDefault), "hipStreamCreateWithFlags");
        *hip_stream = s;
        SHL_CATCH
    }
    SHL_FUNC shl_stream_destroy(void *hip_stream)
    {
        SHL_TRY
        hip_ok(hipStreamSynchronize((hipStream_t)hip_stream), "hipStreamSynchronize");
        hip_ok(hipStreamDestroy((hipStream_t)hip_stream), "hipStreamDestroy");
        SHL_CATCH
    }
    SHL_FUNC shl_malloc(uint64_t bytes, void **device_ptr)
    {
        IfNullRet(device_ptr, SHL_E_POINTER);
        SHL_TRY
        if (hipMalloc(device_ptr, bytes) != hipSuccess)
            throw std::bad_alloc();
        SHL_CATCH
    }
    SHL_FUNC shl_free(void *device_ptr)
    {
        SHL_TRY
        hip_ok(hipFree(device_ptr), "hipFree");
        SHL_CATCH
    }
    SHL_FUNC shl_memcpy_h2d(void *device_dst, const void *host_src, uint64_t bytes)
    {
        SHL_TRY
        hip_ok(hipMemcpy(device_dst, host_src, bytes, hipMemcpyHostToDevice), "H2D");
        SHL_CATCH
    }
    SHL_FUNC shl_memcpy_d2h(void *host_dst, const void *device_src, uint64_t bytes)
    {
        SHL_TRY
        hip_ok(hipDeviceSynchronize(), "sync");
        hip_ok(hipMemcpy(host_dst, device_src, bytes, hipMemcpyDeviceToHost), "D2H");
        SHL_CATCH
    }
    SHL_FUNC shl_device_synchronize(void)
    {
        SHL_TRY
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        SHL_CATCH
    }
    SHL_FUNC shl_timer_create(void **timer)
    {
        IfNullRet(timer, SHL_E_POINTER);
        SHL_TRY
        auto t = new Timer();
        hip_ok(hipEventCreate(&t->e0), "hipEventCreate");
        hip_ok(hipEventCreate(&t->e1), "hipEventCreate");
        *timer = t;
        SHL_CATCH
    }
    SHL_FUNC shl_timer_destroy(void *timer)
    {
        IfNullRet(timer, SHL_E_POINTER);
        auto t = as<Timer>(timer);
        (void)hipEventDestroy(t->e0);
        (void)hipEventDestroy(t->e1);
        delete t;
        return SHL_S_OK;
    }
    SHL_FUNC shl_timer_start(void *timer, void *stream)
    {
        IfNullRet(timer, SHL_E_POINTER);
        SHL_TRY
        hip_ok(hipEventRecord(as<Timer>(timer)->e0, (hipStream_t)stream), "hipEventRecord");
        SHL_CATCH
    }
    SHL_FUNC shl_timer_stop(void *timer, void *stream, float *milliseconds)
    {
        IfNullRet(timer, SHL_E_POINTER);
        IfNullRet(milliseconds, SHL_E_POINTER);
        SHL_TRY
        auto t = as<Timer>(timer);
        hip_ok(hipEventRecord(t->e1, (hipStream_t)stream), "hipEventRecord");
        hip_ok(hipEventSynchronize(t->e1), "hipEventSynchronize");
        hip_ok(hipEventElapsedTime(milliseconds, t->e0, t->e1), "hipEventElapsedTime");
        SHL_CATCH
    }
}
