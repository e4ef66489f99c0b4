// Host orchestration: the device-resident counterparts of seal::Ciphertext, seal::KSwitchKeys and
// seal::Evaluator for the hot path.  Same method names, argument meaning, metadata updates and
// exception classes as the reference (native/src/seal/evaluator.h:79-1387, evaluator.cpp); the
// arithmetic is enqueued on a HIP stream as the kernels of ntt_kernels.hip / poly_kernels.hip /
// behz_kernels.hip.
#pragma once
#include "context.h"
#include "poly_kernels.h"
#include "pool.h"
#include "comm.h"
#include "ntt2_kernels.h"
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace sealhip
{
    // A batch of `batch` ciphertexts sharing metadata; slab layout [poly][batch][K][N].
    class Evaluator;
    // A key-switch tail that has not run yet (Evaluator::switch_key_inplace and the digit-parallel switch_key_finish; CKKS and BFV at
    // the two-pass sizes): the two planes of the ciphertext still hold the addends, `acc` the key-switch sums [batch][2][K+1][N].
    // Whoever touches the words next completes it - except, on the same evaluator, CKKS rescale_to_next_inplace and BFV
    // mod_switch_to_next_inplace, which fold the mod-down and their own division into one pass (ntt_kernels.h: NttTail2;
    // switch_key_finish_modswitch_bfv).  Results are the same words either way.
    struct LazyTail
    {
        const Evaluator *owner;
        uint64_t *acc;
        // CKKS on the fused path: the data-prime components of acc are c + S P^-1 already (ntt2_kernels.h: KsFusedArgs::fold_c0) -
        // the tail, folded into a rescale or not, reads one operand where it read two
        bool with_addend = false;
    };
    // A CKKS 2 x 2 tensor product that has not been formed yet (round 6; Evaluator::multiply into a third object, multiply_inplace and
    // square_inplace; batches large enough for the un-split key switch, two-pass sizes): the destination has its shape and metadata, its
    // words are pending.  A
    // relinearize_inplace on the same evaluator then never stores the product: the third polynomial is formed inside the inverse
    // transform that opens the key switch (NttBatch::prod_x), the first two inside the key switch's last epilogue
    // (KsFusedArgs::fold_x) - one kernel and 45 MB per ciphertext less at the headline size.  Anything else that touches the
    // destination's words forms the product first (Ciphertext::settle), and anything that is about to WRITE, re-shape or destroy an
    // operand forms the products that read it first (Ciphertext::before_write): same words either way.  SEALHIP_LAZY_PRODUCT=0 turns
    // the deferral off.
    class Ciphertext;
    struct LazyProduct
    {
        const Evaluator *owner;
        // operands that are live objects; null = that operand's two polynomials are in `own`
        const Ciphertext *x, *y;
        // in-place products (multiply_inplace, square_inplace): the destination's PREVIOUS slab - its two polynomials as they were -
        // belongs to the record until the product is formed, consumed or discarded; the destination itself got a fresh slab of three
        uint64_t *own;
        const uint64_t *xw() const; // plane 0 of operand x (settles whatever is pending on a live operand)
        const uint64_t *yw() const;
    };
    void lazy_product_stats(uint64_t &fused, uint64_t &formed, uint64_t &dropped);
    // rotations that read their operand through the automorphism's index map inside the key switch / that ran the permutation kernels
    void galois_path_stats(uint64_t &gathered, uint64_t &permuted);
    // process-wide counters (tests, tools): tails folded into a rescale / completed on their own / discarded unrun
    void lazy_tail_stats(uint64_t &folded, uint64_t &plain, uint64_t &dropped);
    // chunked key switching (evaluator_keyswitch.cpp): calls that ran in chunks, chunks issued, largest intermediate held since the previous query (words)
    void ks_chunk_stats(uint64_t *calls, uint64_t *chunks, uint64_t *scratch_words_max);

    // ---- what a key switch decides before it launches (evaluator_keyswitch.cpp: Evaluator::ks_route - the one place that decides)
    // chunks of a large batch dealt to forked lanes (evaluator_keyswitch.cpp: ks_plan)
    struct KsPlan
    {
        unsigned chunk; // items per chunk
        unsigned lanes; // streams the chunks are dealt to (1 = everything on the evaluator's stream)
        unsigned chunks(unsigned batch) const { return (batch + chunk - 1) / chunk; }
    };
    struct KsRoute
    {
        bool fused = false; // the key is in register order (which it only is at a two-pass size): ks1t + ks2, not transform + inner product
        unsigned split = 1; // in-launch digit groups (small batches, fused only); `split` sum buffers leave the launch
        bool fold = false;  // CKKS, fused: the sums leave as c + S P^-1 - from ks2's epilogue (split 1) or the pass that adds the groups
        bool defer = false; // CKKS and BFV at the two-pass sizes: the mod-down is left pending (LazyTail)
        KsPlan plan{ 0, 1 };
        unsigned j0 = 0, j1 = 0; // the digits this call sums (a rank's share in the digit-parallel forms, else all K)
        // the un-split folded launch is the only one whose kernels can form or permute their operands as they load them:
        bool takes_product() const { return fused && fold && split == 1; } // may a pending tensor product be consumed here
        bool reads_through_map() const;                                    // may a rotation's operand be read through the index map here
    };
    // What rides along into the sums of an un-split folded key switch (KsFusedArgs::fold_*); anything but nothing() needs such a route.
    struct KsAddend
    {
        bool folds = false;                // false: nothing rides along
        bool c1_zero = false;              // the second polynomial is zero and has NOT been written (always so for a rotation's operand)
        uint32_t galois_elt = 0;           // != 0: c0 and the target are the UNPERMUTED polynomials of a rotation's operand, read
        const uint64_t *c0 = nullptr;      //       through the automorphism's index map; else the ciphertext's own planes
        const LazyProduct *prod = nullptr; // the operands of a tensor product that was never stored, instead of planes
        // a Galois set (ntt_kernels.h: KsSetView; v0 is filled per launch): key - and with set.map element and source item - per virtual
        // item.  With set.map, c0 and the target are the BASE of the unpermuted operand's planes (as galois_elt, per item)
        KsSetView set{};
        static KsAddend nothing() { return {}; }
        static KsAddend planes(bool c1_zero_unwritten = false) { return { true, c1_zero_unwritten, 0, nullptr, nullptr }; }
        static KsAddend galois(uint32_t elt, const uint64_t *operand_c0) { return { true, true, elt, operand_c0, nullptr }; }
        static KsAddend product(const LazyProduct &p) { return { true, false, 0, nullptr, &p }; }
        static KsAddend galois_set(const KsSetView &view, const uint64_t *operand_c0) // the map-reading form
        {
            KsAddend a{ true, true, 0, operand_c0, nullptr };
            a.set = view;
            return a;
        }
        KsAddend with_keys_of(const KsSetView &view) const // permuted operands: only the key is per item
        {
            KsAddend a = *this;
            a.set = view;
            return a;
        }
    };

    class Ciphertext
    {
    public:
        explicit Ciphertext(const Context &ctx, size_t batch = 1) : ctx_(&ctx), batch_(batch ? batch : 1) {}
        ~Ciphertext();
        Ciphertext(const Ciphertext &o);
        Ciphertext &operator=(const Ciphertext &o);

        const Context &context() const { return *ctx_; }
        size_t batch() const { return batch_; }
        size_t size() const { return size_; }
        const Level *level() const { return level_; }
        size_t coeff_modulus_size() const { return level_ ? level_->K : 0; }
        size_t poly_modulus_degree() const { return level_ ? ctx_->n() : 0; }
        bool &is_ntt_form() { return is_ntt_form_; }
        bool is_ntt_form() const { return is_ntt_form_; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        uint64_t &correction_factor() { return correction_factor_; }
        uint64_t correction_factor() const { return correction_factor_; }
        // every access to the words completes a deferred key-switch tail first (LazyTail)
        uint64_t *data()
        {
            settle();
            before_write(); // a mutable pointer is a write as far as pending products of THIS ciphertext's words are concerned
            return data_;
        }
        const uint64_t *data() const
        {
            settle();
            return data_;
        }
        size_t plane_words() const { return level_ ? batch_ * level_->K * ctx_->n() : 0; }
        size_t word_count() const { return size_ * plane_words(); }
        uint64_t *plane(size_t p) { return data() + p * plane_words(); }
        const uint64_t *plane(size_t p) const { return data() + p * plane_words(); }
        bool has_lazy_tail() const { return lazy_ != nullptr; }
        bool has_lazy_product() const { return lazy_prod_ != nullptr; }
        bool has_storage() const { return data_ != nullptr; } // a question about the buffer, not about its words

        // Ciphertext::resize(context, parms_id, size) (ciphertext.cpp:101-116): keeps the leading
        // polynomials when only `size` changes at the same level; contents are unspecified after a
        // level change.  New polynomials are zero (the reference's DynArray zero-fills).
        void resize(const Level *level, size_t size, hipStream_t stream);
        // adopt a freshly computed slab (takes ownership of `words` from the pool)
        void adopt(const Level *level, size_t size, uint64_t *slab, size_t capacity_words);
        // same shape change as resize() but the contents are left undefined (the caller overwrites them)
        void reshape_uninitialized(const Level *level, size_t size);
        size_t capacity_words() const { return capacity_words_; }
        void release();
        // Ciphertext::reserve (ciphertext.cpp:38-78): room for `size_capacity` polynomials at `level`; the size shrinks to the capacity when
        // it was larger, the leading words are kept (at the same level they are the leading polynomials).  2 <= size_capacity <= 16.
        void reserve(const Level *level, size_t size_capacity, hipStream_t stream);
        // Ciphertext::size_capacity (ciphertext.h:520-528): polynomials the slab has room for at the current level
        size_t size_capacity() const { return plane_words() ? capacity_words_ / plane_words() : 0; }
        // sealc Ciphertext_SetParmsId writes the member without any check (c/ciphertext.cpp:239-247); here a level is a pointer into the context
        void set_level_unchecked(const Level *level)
        {
            settle();
            before_write();
            level_ = level;
        }

    private:
        const Context *ctx_;
        size_t batch_;
        size_t size_ = 0;
        const Level *level_ = nullptr;
        bool is_ntt_form_ = false;
        double scale_ = 1.0;
        uint64_t correction_factor_ = 1;
        uint64_t *data_ = nullptr;
        size_t capacity_words_ = 0;
        // deferred key-switch tail (owned; see LazyTail)
        mutable LazyTail *lazy_ = nullptr;
        void settle() const; // run it now
        void drop_lazy();    // the words are about to be replaced: discard it
        // pending tensor product whose destination this is (owned; see LazyProduct), and the pending products that READ this object
        mutable LazyProduct *lazy_prod_ = nullptr;
        mutable std::vector<const Ciphertext *> prod_readers_;
        mutable unsigned prod_reader_count_ = 0; // = prod_readers_.size(), readable without the list's lock
        void settle_product() const;             // form it now
        void drop_product();                     // the words are about to be replaced: discard it
        void before_write() const                // form every pending product that reads this object's words
        {
            if (__atomic_load_n(&prod_reader_count_, __ATOMIC_ACQUIRE))
                settle_readers();
        }
        void settle_readers() const;
        // the slab is replaced by `slab` (uninitialised, room for capacity_words) and handed to the caller instead of the pool
        uint64_t *exchange_slab(const Level *level, size_t size, uint64_t *slab, size_t capacity_words);
        friend class Evaluator;
        friend struct LazyProduct;
        friend void lazy_product_link(const Ciphertext *, const LazyProduct &);
        friend void lazy_product_unlink(const Ciphertext *, const LazyProduct &);
    };

    // LazyProduct bookkeeping (objects.cpp): the reader lists of the live operands, only touched under one global lock
    void lazy_product_link(const Ciphertext *dest, const LazyProduct &p);
    void lazy_product_unlink(const Ciphertext *dest, const LazyProduct &p);

    // seal::Plaintext (plaintext.h) resident in HBM: either coeff_count <= N coefficients modulo t (BFV/BGV,
    // parms_id_zero) or, in NTT form, K*N words at a level (CKKS always; BFV/BGV after transform_to_ntt_inplace).
    // One Plaintext object is applied to every item of a ciphertext batch; one plaintext per item is what the Evaluator's *_device
    // forms take, as raw device words.
    class Plaintext
    {
    public:
        explicit Plaintext(const Context &ctx) : ctx_(&ctx) {}
        ~Plaintext();
        Plaintext(const Plaintext &o);
        Plaintext &operator=(const Plaintext &o);

        const Context &context() const { return *ctx_; }
        size_t coeff_count() const { return coeff_count_; }
        const Level *level() const { return level_; } // parms_id: null = parms_id_zero = not in NTT form
        void set_level(const Level *l) { level_ = l; }
        bool is_ntt_form() const { return level_ != nullptr; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        uint64_t *data() { return data_; }
        const uint64_t *data() const { return data_; }
        // Plaintext::resize (plaintext.h:268-290): new coefficients are zero
        void resize(size_t coeff_count, hipStream_t stream);
        // Plaintext_Set4: coefficient form, `count` words from host or device memory
        void set(const uint64_t *words, size_t count, bool from_device);
        void adopt(uint64_t *slab, size_t count, size_t capacity_words);
        void adopt_count(size_t count) { coeff_count_ = count; } // shrink in place (plaintext mod switching)

    private:
        const Context *ctx_;
        size_t coeff_count_ = 0;
        const Level *level_ = nullptr;
        double scale_ = 1.0;
        uint64_t *data_ = nullptr;
        size_t capacity_words_ = 0;
    };

    // KSwitchKeys::keys_ (kswitchkeys.h:340): per index, `digits` size-2 key-level ciphertexts in NTT
    // form, stored as one slab [digit][2][L][N].
    class KSwitchKeys
    {
    public:
        struct Key
        {
            uint64_t *dev = nullptr;
            size_t digits = 0; // decomposition digits resident in `dev`
            size_t digit0 = 0; // index of the first of them (non-zero only for a digit-parallel slice)
            // true: every component is stored in the register order of the fused key-switch
            // kernel, as doubles for primes of the double-precision back end (ntt2_kernels.h)
            bool register_order = false;
            // which installation of a key this is (process-wide count, never 0 for a resident key): a slab address can come back
            // from the allocator for the next key, a serial cannot (GaloisSet::keys_current)
            uint64_t serial = 0;
        };
        ~KSwitchKeys();
        // words: `digits` digits starting at digit `digit0` of key `index`, each 2 x L x N words
        void set_key(const Context &ctx, size_t index, size_t digits, const uint64_t *words, bool from_device, size_t digit0 = 0);
        // the same with the words delivered by `upload(device_destination)` (e.g. piecewise from a serialized stream)
        void set_key_with(const Context &ctx, size_t index, size_t digits, const std::function<void(uint64_t *)> &upload, size_t digit0 = 0);
        // the words of key `index` as set_key took them ([digits][2][L][N], canonical, natural order), written to device memory
        void key_words(size_t index, uint64_t *device_out) const;
        // one digit of key `index` ([2][L][N] words, as key_words): the transient conversion buffer of a save is one digit, not a key
        void digit_words(size_t index, size_t digit, uint64_t *device_out) const;
        // HBM held by the keys (register order: ntt2_kernels.h - a C5 key is 284 MB, its natural words 252 MB)
        size_t device_bytes() const;
        void clear(); // drop every key (KSwitchKeys::load replaces the whole object, kswitchkeys.cpp:92-180)
        bool has_key(size_t index) const { return index < keys_.size() && keys_[index].dev != nullptr; }
        const Key &key(size_t index) const { return keys_[index]; }
        size_t slots() const { return keys_.size(); }
        // KSwitchKeys::data().size() of the reference object: N for GaloisKeys (galoiskeys.h), what a stream said for a loaded one
        void reserve_slots(size_t count)
        {
            if (keys_.size() < count)
                keys_.resize(count);
        }
        size_t size() const;
        const Context *context() const { return ctx_; }
        // KSwitchKeys::operator= (kswitchkeys.h:74-101): a deep copy, every key slab duplicated in HBM
        void assign(const KSwitchKeys &other);
        // KSwitchKeys::parms_id (kswitchkeys.h:169-183): the key level's once a key is installed, unless the caller wrote another
        void get_parms_id(uint64_t *out) const;
        void set_parms_id(const uint64_t *id);

    private:
        std::vector<Key> keys_;
        const Context *ctx_ = nullptr;
        uint64_t parms_id_[4] = { 0, 0, 0, 0 };
        bool parms_id_written_ = false;
        size_t key_bytes(const Key &k) const;
    };

    // A device-resident CSR list of item numbers (include/sealhip.h: ItemMap_Create): which items of a batch, or which pairs of
    // items of two, the terms of each output item of a mapped reduction are.  Validated once, at construction (std::invalid_argument);
    // uploaded once as 32-bit words, each list 16-byte aligned in one pool block, with a synchronous copy after a device drain.  The
    // reductions read the lists from HBM, so one map serves many calls and recordings.  The destructor hands the block back to the
    // stream-aware pool (pool.h) outside any stream scope, i.e. tagged "unknown": its next user first waits for every registered
    // stream and the NULL stream, so a map may be destroyed while work that reads it is still queued - nothing is drained here.
    struct ItemWalk;
    struct Conv2dShape;
    class ItemMap
    {
    public:
        ItemMap(const Context &context, uint64_t rows, const uint64_t *row_offsets, const uint64_t *first_items, const uint64_t *second_items,
                uint64_t first_batch, uint64_t second_batch);
        ~ItemMap();
        ItemMap(const ItemMap &) = delete;
        ItemMap &operator=(const ItemMap &) = delete;
        const Context *context() const { return ctx_; }
        size_t rows() const { return rows_; }
        size_t terms() const { return terms_; }
        size_t longest_row() const { return longest_; }
        size_t first_batch() const { return first_batch_; }
        size_t second_batch() const { return second_batch_; }
        bool one_list() const { return first_ == second_; }
        ItemWalk walk() const;

    private:
        const Context *ctx_;
        size_t rows_, terms_ = 0, longest_ = 0, first_batch_, second_batch_;
        uint64_t *block_ = nullptr;
        const uint32_t *offsets_ = nullptr, *first_ = nullptr, *second_ = nullptr;
    };

    // A Galois set (include/sealhip.h: GaloisSet_Create): R Galois elements whose automorphisms one call applies to every item of a
    // batch (Evaluator::apply_galois_set).  The counterpart of ItemMap: validated once (std::invalid_argument), uploaded once - one
    // KsSetEntry (ntt_kernels.h) per entry that is not the identity, with a synchronous copy after a device drain - and read from HBM
    // by the key switch's per-item kernels, so one set serves many calls and recordings.  An element of 0 is an identity entry (a
    // step of 0): a copy, never key-switched.  The keys object must outlive the set; a call checks on the host that every recorded
    // key slab is still the key's current one.  The destructor follows ItemMap's pool rule.
    class GaloisSet
    {
    public:
        GaloisSet(const Context &context, const KSwitchKeys &galois_keys, uint64_t count, const uint32_t *galois_elts, bool zero_is_identity);
        ~GaloisSet();
        GaloisSet(const GaloisSet &) = delete;
        GaloisSet &operator=(const GaloisSet &) = delete;
        const Context *context() const { return ctx_; }
        const KSwitchKeys &keys() const { return *keys_; }
        size_t count() const { return elts_.size(); }
        size_t switched() const { return entry_of_.size(); } // entries that are not the identity
        uint32_t elt(size_t r) const { return elts_[r]; }
        size_t entry_of(size_t i) const { return entry_of_[i]; } // the entry the i-th table row stands for
        size_t distinct() const { return distinct_; }
        bool register_order() const { return register_order_; }
        const KsSetEntry *table() const { return table_; }
        bool keys_current() const; // every recorded slab is still the key's
        bool full_keys(size_t digits) const; // every key holds the digits [0, digits)

    private:
        const Context *ctx_;
        const KSwitchKeys *keys_;
        std::vector<uint32_t> elts_;
        std::vector<size_t> entry_of_;
        std::vector<const uint64_t *> slabs_; // per table row: the key's slab and the serial of its installation
        std::vector<uint64_t> serials_;
        size_t distinct_ = 0;
        bool register_order_ = true;
        uint64_t *block_ = nullptr;
        const KsSetEntry *table_ = nullptr;
    };
    // set calls served by the one-batch route / by the loop over the entries; fused key-switch launches issued by set calls
    void galois_set_stats(uint64_t &batched, uint64_t &looped, uint64_t &fused_launches);
    void galois_set_count_fused_launch();

    class Evaluator
    {
    public:
        explicit Evaluator(const Context &context);
        ~Evaluator();

        const Context &context() const { return context_; }
        // work of this evaluator is enqueued on `s` (nullptr = the NULL stream); the stream is registered with the device
        // pool so that memory recycled between evaluators on different streams is ordered (pool.h)
        void set_stream(hipStream_t s);
        hipStream_t stream() const { return stream_; }
        void synchronize() const;
        // SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT (evaluator.cpp:386-392) needs a device->host round trip
        // per operation; off by default for device-resident batches, on for drop-in parity checks.
        void set_transparent_check(bool on) { transparent_check_ = on; }

        void negate_inplace(Ciphertext &encrypted) const;
        void add_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2) const;
        void sub_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2) const;
        void multiply_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2) const;
        void multiply(const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination) const;
        void square_inplace(Ciphertext &encrypted) const;
        void relinearize_inplace(Ciphertext &encrypted, const KSwitchKeys &relin_keys) const;
        void mod_switch_to_next_inplace(Ciphertext &encrypted) const;
        void mod_switch_to_inplace(Ciphertext &encrypted, const uint64_t *parms_id) const;
        void rescale_to_next_inplace(Ciphertext &encrypted) const;
        void rescale_to_inplace(Ciphertext &encrypted, const uint64_t *parms_id) const;
        void mod_reduce_to_next_inplace(Ciphertext &encrypted) const;
        void mod_reduce_to_inplace(Ciphertext &encrypted, const uint64_t *parms_id) const;
        void transform_to_ntt_inplace(Ciphertext &encrypted) const;
        // plaintext operands and the many-operand forms (evaluator.cpp:242-261, 1649-2287, 1369-1402)
        void add_plain_inplace(Ciphertext &encrypted, const Plaintext &plain) const;
        void sub_plain_inplace(Ciphertext &encrypted, const Plaintext &plain) const;
        void multiply_plain_inplace(Ciphertext &encrypted, const Plaintext &plain) const;
        void transform_to_ntt_inplace(Plaintext &plain, const uint64_t *parms_id) const;
        void mod_switch_to_next_inplace(Plaintext &plain) const;
        void mod_switch_to_inplace(Plaintext &plain, const uint64_t *parms_id) const;
        // One plaintext PER ITEM of a device-resident batch (include/sealhip.h: Evaluator_AddPlainDevice ...): plain = `batch` plaintexts
        // in device memory, [batch][N] coefficients modulo t (plain_is_ntt false; BFV / BGV) or [batch][K][N] NTT-form words at the
        // ciphertext's level (plain_is_ntt true; CKKS always), item b for item b of `encrypted`.  Item b of the result equals, word for
        // word, add_plain_inplace / sub_plain_inplace / multiply_plain_inplace on a batch of one with plaintext b; the form checks,
        // metadata updates and exception classes are theirs.  destination may be encrypted (in place); otherwise encrypted is only
        // read and a call that fails its checks leaves destination untouched.  `scale`: the plaintexts' common scale (CKKS).
        void add_plain_device(const Ciphertext &encrypted, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                              Ciphertext &destination) const;
        void sub_plain_device(const Ciphertext &encrypted, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                              Ciphertext &destination) const;
        void multiply_plain_device(const Ciphertext &encrypted, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                   Ciphertext &destination) const;
        // transform_to_ntt_inplace(Plaintext) for `batch` plaintexts: [batch][N] coefficients modulo t -> [batch][K][N] NTT-form words
        // at parms_id (centred lift, forward transform); BFV / BGV
        void transform_plain_to_ntt_device(const uint64_t *coefficients, size_t batch, const uint64_t *parms_id, uint64_t *words) const;
        // Reductions over the ITEMS of a device-resident batch (include/sealhip.h: Evaluator_SumItems / Evaluator_DotPlainDevice;
        // batch_reduce_kernels.h).  `group` divides encrypted's batch B; destination is another object whose batch is B / group; item o
        // of it becomes the sum of the items o * group .. o * group + group - 1 - word for word add_many over batches of one holding
        // them - or, for dot_plain_device, of their products with the NTT-form plaintexts plain [B][K][N] (multiply_plain_device with
        // plain_is_ntt = true, then that sum; scale handling and bound check are its).  encrypted is only read; a call that fails
        // its checks leaves destination untouched.
        void sum_items(const Ciphertext &encrypted, size_t group, Ciphertext &destination) const;
        void dot_plain_device(const Ciphertext &encrypted, const uint64_t *plain, size_t batch, size_t group, double scale,
                              Ciphertext &destination) const;
        // The ciphertext x ciphertext reduction (include/sealhip.h: Evaluator_DotItems): item o of destination becomes the sum over the
        // items o * group .. o * group + group - 1 of the 2 x 2 tensor products encrypted1_b (x) encrypted2_b - word for word multiply
        // on batches of one and add_many over the products, without storing a product.  CKKS and BGV, both operands of size 2 and in
        // NTT form; encrypted1 and encrypted2 may be the same object; destination is another object (size 3 afterwards).
        void dot_items(const Ciphertext &encrypted1, const Ciphertext &encrypted2, size_t group, Ciphertext &destination) const;
        // The same three reductions over the items an ItemMap names (include/sealhip.h: Evaluator_SumItemsMapped ...): item o of
        // destination, a batch of map.rows() items, is the sum over the terms t of row o of encrypted_first[t], of
        // encrypted_first[t] (.) plain_second[t], or of encrypted1_first[t] (x) encrypted2_second[t].  Checks, metadata, settling and
        // words are those of the forms above on the named items; encrypted's batch is the map's first_batch, the plaintexts' count /
        // encrypted2's batch its second_batch.
        void sum_items_mapped(const Ciphertext &encrypted, const ItemMap &map, Ciphertext &destination) const;
        void dot_plain_mapped(const Ciphertext &encrypted, const uint64_t *plain, size_t plain_count, const ItemMap &map, double scale,
                              Ciphertext &destination) const;
        void dot_items_mapped(const Ciphertext &encrypted1, const Ciphertext &encrypted2, const ItemMap &map, Ciphertext &destination) const;
        // dot_plain_mapped with scalar weights in either form of matmul_scalars_items (include/sealhip.h: Evaluator_DotScalarsMapped)
        void dot_scalars_mapped(const Ciphertext &encrypted, const void *weights, size_t weight_count, bool narrow, const ItemMap &map,
                                double scale, Ciphertext &destination) const;
        // Ciphertext matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulItems): item i * cols + j of destination, a batch
        // of rows * cols items, becomes the sum over k < inner of encrypted1_(i * inner + k) (x) encrypted2_(k * cols + j) - item
        // j * inner + k of encrypted2 when second_transposed - word for word dot_items_mapped over the dense pair map; checks,
        // metadata and settling are dot_items'.  A kernel of its own, whose threads hold a tile of output rows x columns
        // (batch_reduce_kernels.h: k_matmul_items)
        void matmul_items(const Ciphertext &encrypted1, const Ciphertext &encrypted2, size_t rows, size_t inner, size_t cols,
                          bool second_transposed, Ciphertext &destination) const;
        // Plaintext matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulPlainItems): item i * cols + j of destination, a
        // batch of rows * cols items - item j * rows + i when result_transposed -, becomes the sum over k < inner of plaintext
        // i * inner + k times encrypted_(k * cols + j) - item j * inner + k when second_transposed - word for word dot_plain_mapped
        // over the dense map; checks, metadata and settling are dot_plain_device's.  plain: [rows * inner][K][N] NTT-form device
        // words at encrypted's level.  A kernel of its own, whose threads hold a tile of output rows x columns
        // (batch_reduce_kernels.h: k_matmul_plain_items)
        void matmul_plain_items(const uint64_t *plain, const Ciphertext &encrypted, size_t rows, size_t inner, size_t cols,
                                bool second_transposed, bool result_transposed, double scale, Ciphertext &destination) const;
        // Scalar weight matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulScalarsItems): matmul_plain_items with the
        // plaintext i * inner + k being the constant whose K words are weights[i * inner + k] ([rows * inner][K] device words) or,
        // narrow, the constant polynomial with the signed 32-bit integer value weights[i * inner + k] ([rows * inner] of them) - word
        // for word matmul_plain_items with the weights expanded to [K][N]; checks, metadata and settling are dot_plain_device's.
        // weights: written earlier on the stream.  A kernel of its own (batch_reduce_kernels.h: k_matmul_scalars)
        void matmul_scalars_items(const void *weights, bool narrow, const Ciphertext &encrypted, size_t rows, size_t inner, size_t cols,
                                  bool second_transposed, bool result_transposed, double scale, Ciphertext &destination) const;
        // 2-D convolution of scalar weights over a grid of items (include/sealhip.h: Evaluator_Conv2dScalarsItems): encrypted is a
        // batch of C * H * W items, destination one of OC * OH * OW, weights [OC][C * kh * kw] in either form of
        // matmul_scalars_items; output item (o, y', x') is the sum over the taps inside the image - word for word dot_plain_mapped
        // over the map of those taps with the weights expanded to [K][N]; checks, metadata and settling are matmul_scalars_items'.
        // in_last / out_last: the channel is the fastest index of the input / result.  No gathered batch is made
        // (batch_reduce_kernels.h: k_conv2d_scalars)
        void conv2d_scalars_items(const void *weights, bool narrow, const Ciphertext &encrypted, const Conv2dShape &shape, bool in_last,
                                  bool out_last, double scale, Ciphertext &destination) const;
        // A dense rows x batch matrix of SCALAR plaintexts times the items of a batch (include/sealhip.h: Evaluator_DotScalarsDevice):
        // item o of destination, a batch of `rows` items, becomes the sum over b of encrypted_b times the constant plaintext whose K
        // words are scalars[o][b] - word for word dot_plain_mapped over the dense map with the scalars expanded to [K][N]; checks,
        // metadata and settling are dot_plain_device's.  scalars: [rows][batch][K] device words, written earlier on the stream
        void dot_scalars_device(const Ciphertext &encrypted, const uint64_t *scalars, size_t rows, size_t batch, double scale,
                                Ciphertext &destination) const;
        // BFV / BGV: host values modulo t -> [count][K] device words, scalar i = what transform_plain_to_ntt_device leaves at every
        // coefficient for the constant polynomial values[i] (one synchronous copy after a drain; not a hot-path call)
        void lift_scalars(size_t count, const uint64_t *values_mod_t, const uint64_t *parms_id, uint64_t *device_words) const;
        void add_many(const std::vector<const Ciphertext *> &encrypteds, Ciphertext &destination) const;
        void multiply_many(const std::vector<const Ciphertext *> &encrypteds, const KSwitchKeys &relin_keys, Ciphertext &destination) const;
        void exponentiate_inplace(Ciphertext &encrypted, uint64_t exponent, const KSwitchKeys &relin_keys) const;
        void transform_from_ntt_inplace(Ciphertext &encrypted_ntt) const;
        void apply_galois_inplace(Ciphertext &encrypted, uint32_t galois_elt, const KSwitchKeys &galois_keys) const;
        // out-of-place forms (evaluator.h:1072-1315 of the reference): with the exact Galois key present `encrypted` is read where
        // it lies - no copy into the destination first
        void apply_galois(const Ciphertext &encrypted, uint32_t galois_elt, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        // include/sealhip.h: Evaluator_ApplyGaloisSet - item b R + r of `destination` (batch B R, another object) = apply_galois of item b
        // with entry r; an identity entry is a copy
        void apply_galois_set(const Ciphertext &encrypted, const GaloisSet &set, Ciphertext &destination) const;
        void rotate_rows(const Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        void rotate_columns(const Ciphertext &encrypted, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        void rotate_vector(const Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        void complex_conjugate(const Ciphertext &encrypted, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        // in place = the operand as destination
        void rotate_rows_inplace(Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys) const;
        void rotate_columns_inplace(Ciphertext &encrypted, const KSwitchKeys &galois_keys) const;
        void rotate_vector_inplace(Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys) const;
        void complex_conjugate_inplace(Ciphertext &encrypted, const KSwitchKeys &galois_keys) const;

        bool is_transparent(const Ciphertext &ct) const; // synchronises

        // hipGraph capture of a fixed operation sequence.  Between begin_capture() and end_capture() the
        // operations issued on this evaluator are RECORDED (stream capture, side streams included), not executed; the returned
        // executable graph replays them with one launch on the same device buffers - operands, destinations and scratch keep
        // the addresses they had during capture, so the caller refreshes the operands' contents in place and reads the
        // destinations after each replay.  Run the sequence once eagerly first (lazily built tables, pool warm-up), keep the
        // captured objects alive and do not resize them between replays.  At small batches the step is launch-bound on the
        // host (about 25 kernel launches + stream fork/join per multiply+relinearize+rescale): see profiles/HISTORY.md section 5 ("Small batches / latency").
        // an executable graph together with the scratch blocks whose addresses it replays on (kept out of the pool until
        // the graph is destroyed)
        struct Graph
        {
            hipGraphExec_t exec = nullptr;
            std::vector<uint64_t *> scratch;
            ~Graph();
        };
        void begin_capture();
        Graph *end_capture();
        void launch_graph(const Graph *graph) const;

        static size_t relin_index(size_t key_power);       // RelinKeys::get_index  (relinkeys.h:58)
        static size_t galois_index(uint32_t galois_elt);   // GaloisKeys::get_index (galoiskeys.h:48)
        uint32_t galois_elt_from_step(int step) const;      // GaloisTool::get_elt_from_step (galois.cpp:53)

        // the two halves of switch_key_inplace for digit-parallel key switching over several GPUs:
        // acc = [batch][2][K+1][N] words (switch_key_acc_words); partial fills it with the canonical partial sums of
        // the digits [j0, j1); finish reduces the sum of `parts` such buffers and applies the mod-down to encrypted.
        size_t switch_key_acc_words(const Ciphertext &encrypted) const;
        // relinearize (size 3 -> 2) and apply_galois (size 2) split the same way: *_partial leaves `encrypted` ready for
        // the finish call (for apply_galois: c0 <- pi(c0), c1 <- 0) and writes this rank's partial sums to acc
        void relinearize_partial(Ciphertext &encrypted, const KSwitchKeys &relin_keys, unsigned j0, unsigned j1, uint64_t *acc) const;
        void relinearize_finish(Ciphertext &encrypted, uint64_t *acc, unsigned parts) const;
        void apply_galois_partial(Ciphertext &encrypted, uint32_t galois_elt, const KSwitchKeys &galois_keys, unsigned j0, unsigned j1,
                                  uint64_t *acc) const;
        void apply_galois_finish(Ciphertext &encrypted, uint64_t *acc, unsigned parts) const;

        // ---- digit-parallel key switching with the exchange INSIDE the library: RCCL calls on this
        // evaluator's stream, no host synchronisation.  Every rank of `comm` calls the same method with equal ciphertexts and
        // a key that holds (at least) its own digits comm_split(K, size, rank).  Two exchange shapes:
        //   all_reduce      one all-reduce of the 2(K+1)N partial sums per ciphertext; every rank runs the whole mod-down
        //   reduce_scatter  (CKKS) the sums of the K data moduli are reduce-scattered by owner (comm_split(K, size, rank)),
        //                   the special-prime component is all-reduced, every rank runs the mod-down of ITS moduli only and
        //                   the increments are all-gathered: same bytes on the wire, 1/size of the mod-down per rank
        // Results are bit-identical to the single-GPU operations.  BFV / BGV use the all-reduce shape in either mode.
        enum class KsExchange
        {
            all_reduce = 0,
            reduce_scatter = 1,
        };
        void relinearize_inplace(Ciphertext &encrypted, const KSwitchKeys &relin_keys, Comm &comm, KsExchange how) const;
        void apply_galois_inplace(Ciphertext &encrypted, uint32_t galois_elt, const KSwitchKeys &galois_keys, Comm &comm, KsExchange how) const;
        void rotate_vector_inplace(Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys, Comm &comm, KsExchange how) const;
        // one-time distribution of a key-switching key: rank `root` holds the full key `index`, every rank ends up with its own
        // digits resident (the key is broadcast in its natural layout and re-laid out locally)
        // (staging: a device buffer of K * 2 * L * N words on EVERY rank; on `root` it holds the key [digit][2][L][N])
        void broadcast_key_digits(KSwitchKeys &keys, size_t index, uint64_t *staging, Comm &comm, int root) const;
        // the three local phases of the reduce-scatter shape (the parity tests emulate the ranks in one process):
        //   slots          m = ceil(K / nranks) moduli slots per rank
        //   pack_targets   acc (this rank's partial sums) -> send [nranks][m][batch][2][N] + sp [batch][2][N] (special prime)
        //   finish_owned   recv = the summed chunk of `rank` [m][batch][2][N], sp = the summed special component
        //                  -> own [m][batch][2][N]: the increments of this rank's moduli
        //   add_gathered   all [nranks][m][batch][2][N] -> encrypted += increments
        unsigned switch_key_slots(const Ciphertext &encrypted, unsigned nranks) const;
        void switch_key_pack_targets(const Ciphertext &encrypted, const uint64_t *acc, unsigned nranks, uint64_t *send, uint64_t *sp) const;
        void switch_key_finish_owned(
            const Ciphertext &encrypted, const uint64_t *recv, const uint64_t *sp, unsigned nranks, unsigned rank, uint64_t *own) const;
        void switch_key_add_gathered(Ciphertext &encrypted, const uint64_t *all, unsigned nranks) const;

    private:
        friend class Encryptor; // public-key encryption ends with one modulus switch from the level above (encryptor.cpp:139-186)
        void check_valid(const Ciphertext &ct, const char *what) const;
        void check_context(const Ciphertext &ct, const char *what = "encrypted") const; // of this context and at a level: the walkers' and rotations' check
        void check_batching() const;
        void check_native_form(const Ciphertext &ct) const; // coefficient form for BFV, NTT form for CKKS and BGV
        bool scale_within_bounds(double scale, const Level &lvl) const;
        // the level parms_id names, refused when there is none or it lies above `level` (the *_to walkers)
        const Level *target_level(const Level *level, const uint64_t *parms_id) const;
        void addsub(Ciphertext &e1, const Ciphertext &e2, int op) const; // op 0 add, 1 sub
        void check_product_operands(const Ciphertext &e1, const Ciphertext &e2) const; // both valid, one level, one batch
        size_t product_size(size_t size1, size_t size2) const;                         // -> size1 + size2 - 1, refused outside 3 .. 16
        void check_matmul_shape(size_t rows, size_t inner, size_t cols) const;
        void bfv_multiply_to(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &dst) const;
        void bgv_multiply(Ciphertext &e1, const Ciphertext &e2) const;
        void check_valid(const Plaintext &plain) const;
        // plaintext operands (evaluator.cpp): a Plaintext handle or raw device words with one plaintext per item, one code path
        struct PlainOperand;
        void addsub_plain(const Ciphertext &encrypted, const PlainOperand &plain, int op, Ciphertext &destination) const;
        void multiply_plain(const Ciphertext &encrypted, const PlainOperand &plain, Ciphertext &destination) const;
        template <class Use>
        void lift_chunks(const PlainOperand &plain, const Level &lvl, uint64_t scale_by, size_t batch, uint64_t *out, Use use) const;
        // what add_plain / sub_plain accept per scheme (shared by the per-object and the per-item forms)
        void check_addsub_plain_forms(const Ciphertext &encrypted, bool plain_is_ntt, const Level *plain_level, double plain_scale) const;
        // per_item: one plaintext per item of encrypted (batch must be its batch); otherwise `batch` plaintexts that a map names.
        // scalar_rows: the operand is [scalar_rows][batch][K] words of scalars and not `batch` plaintexts - or, narrow_scalars,
        // [scalar_rows][batch] 32-bit integers
        void check_plain_device(const Ciphertext &encrypted, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                const Ciphertext &destination, bool per_item = true, size_t scalar_rows = 0, bool narrow_scalars = false) const;
        uint64_t *begin_result(const Ciphertext &encrypted, Ciphertext &destination) const; // destination shaped like encrypted, words undefined
        // the walk of consecutive groups (group divides the batch) or of a map (whose first_batch is the batch); -> its output items
        ItemWalk consecutive_walk(const Ciphertext &encrypted, size_t group, size_t &rows) const;
        ItemWalk mapped_walk(const Ciphertext &encrypted, const ItemMap &map, size_t &rows) const;
        void check_reduce_items(const Ciphertext &encrypted, size_t rows, const Ciphertext &destination) const;
        // destination <- `size` planes of `rows` items with this metadata, filled by launch(slices, scratch)
        template <class Launch>
        void reduce_items(const Ciphertext &encrypted, size_t rows, const ItemWalk &walk, size_t size, size_t threads, bool ntt_form,
                          double scale, uint64_t correction_factor, Ciphertext &destination, const char *what, Launch launch) const;
        size_t reduce_threads(const Ciphertext &encrypted, size_t rows, size_t grid_planes) const;
        double check_dot_plain(const Ciphertext &encrypted, size_t rows, double scale, const Ciphertext &destination) const;
        void sum_items(const Ciphertext &encrypted, size_t rows, const ItemWalk &walk, Ciphertext &destination) const;
        void dot_plain_items(const Ciphertext &encrypted, const uint64_t *plain, size_t plain_count, size_t rows, const ItemWalk &walk,
                             double scale, Ciphertext &destination) const;
        // what the ciphertext x ciphertext sums over `rows` output items check once their operands are known: -> the result's
        // scale and correction factor
        void check_dot_items(const Ciphertext &encrypted1, const Ciphertext &encrypted2, size_t rows, const Ciphertext &destination,
                             double &scale, uint64_t &correction_factor) const;
        void dot_items(const Ciphertext &encrypted1, const Ciphertext &encrypted2, size_t rows, const ItemWalk &walk,
                       Ciphertext &destination) const;
        void bgv_correct_and_combine(
            Scratch &delta, const uint64_t *a, size_t a_stride, const ShoupOp *mul, unsigned ncomp, size_t items, uint64_t *out0,
            uint64_t *out1, size_t out_stride, int epi) const;
        void ckks_multiply(Ciphertext &e1, const Ciphertext &e2) const;
        // e1 <- the NTT-domain tensor product of e1 and e2, `size` polynomials (ckks_multiply, bgv_multiply)
        void tensor_ntt(Ciphertext &e1, const Ciphertext &e2, size_t size) const;
        void mod_switch_scale_to_next(Ciphertext &encrypted) const;
        void mod_switch_drop_to_next(Ciphertext &encrypted) const;
        void rotate_internal(Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys) const;
        void rotate_internal(const Ciphertext &encrypted, int steps, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        // rotate_columns and complex_conjugate: the automorphism of step 0 (element 2N - 1), each for the schemes it serves
        void conjugate(bool scheme_served, const Ciphertext &encrypted, const KSwitchKeys &galois_keys, Ciphertext &destination) const;
        void throw_if_transparent(const Ciphertext &ct) const;
        // ---- the key switch proper (evaluator_keyswitch.cpp).  ks_route decides everything once; the callers branch on it and hand the same
        // object down.  digit_parallel: the sums of [j0, j1) leave for the caller's exchange - one group, nothing folded, no tail here.
        KsRoute ks_route(const Level &lvl, size_t batch) const; // the half no key changes: defer, and fold as a register-order key would
        KsRoute ks_route(const Level &lvl, size_t batch, const KSwitchKeys &keys, size_t key_index, unsigned j0, unsigned j1,
                         bool digit_parallel = false) const;
        unsigned ks_shape_split(const Level &lvl, size_t batch) const; // digit groups a batch of this shape would run in (before cap and override)
        // switch_key_inplace (evaluator.cpp:2561): encrypted (size >= 2) += KS(target), target = one plane [batch][K][N] in the scheme's
        // native form.  `addend` says what the caller HAS (its own planes, c1 possibly zero and unwritten - zeroed here only when
        // somebody is going to read it; or a rotation's unpermuted operand); the route says whether it is folded.
        void switch_key_inplace(Ciphertext &encrypted, const uint64_t *target, const KSwitchKeys &keys, size_t key_index, const KsRoute &route,
                                const KsAddend &addend = KsAddend::planes()) const;
        // its two halves.  partial: acc = route.split buffers of [batch][2][K+1][N] words (switch_key_acc_words) <- the canonical partial
        // sums of the digits [route.j0, route.j1), each group's in its own buffer (KsFusedArgs::parts), `addend` folded in.  With a
        // product `target` only names the third polynomial: it is formed from the operands where it is used.
        void switch_key_partial(const Ciphertext &encrypted, const uint64_t *target, const KSwitchKeys &keys, size_t key_index, uint64_t *acc,
                                const KsRoute &route, const KsAddend &addend = KsAddend::nothing()) const;
        // finish: reduces the sum of `parts` buffers and applies the mod-down to encrypted.  acc_has_addend: the sums were folded.
        // may_defer (the digit-parallel finishes): where the route defers and folds, the pass that reduces the sums adds the ciphertext's
        // words into a block of the pool's and the mod-down stays pending; `acc` is not referenced after the call returns
        void switch_key_finish(Ciphertext &encrypted, uint64_t *acc, unsigned parts, bool acc_has_addend = false, bool may_defer = false) const;
        void switch_key_exchange_finish(Ciphertext &encrypted, uint64_t *acc, Comm &comm, KsExchange how) const;
        const uint32_t *ks_comp_prime(unsigned K) const;
        int ks_class_hint(unsigned K) const;
        struct KsTargets
        {
            uint32_t *dev = nullptr; // [targets1: int, fp | targets2: int, fp]
            unsigned n_int = 0, n_fp = 0;
        };
        const KsTargets &ks_targets(unsigned K) const;

        const Context &context_;
        // The stream this evaluator's work is enqueued on, and THE RULE for StreamScope (pool.h tags a freed block with the calling
        // thread's scope stream, so pool traffic of a call has to happen under a scope on stream_ whichever thread calls).  A method
        // opens `StreamScope pool_scope(stream_)` only if it can be the outermost Evaluator call on a thread:
        //   * the public methods - the C layer calls them, and so does the Encryptor (decryptor.cpp: evaluator_), outside any scope;
        //     one that only checks and forwards to another public method needs none;
        //   * mod_switch_scale_to_next - private, but the Encryptor calls it directly as a friend;
        //   * the hooks a Ciphertext calls from arbitrary host code through settle(), drop_*() or its destructor: complete_tail,
        //     forget_tail, complete_product, forget_product.
        // Every other private method only runs under one of these and opens none; one that allocates from or frees to the pool
        // begins with expect_scope() instead, so the emulated build checks the rule on every path the CPU suite runs.
        hipStream_t stream_ = nullptr;
        void expect_scope() const
        {
#ifdef SEALHIP_CHECK_BOUNDS
            if (!(DevicePool::thread_has_scope() && DevicePool::thread_stream() == stream_))
                throw std::logic_error("an Evaluator helper ran outside a StreamScope on the evaluator's stream (evaluator.h: stream_)");
#endif
        }
        hipStream_t capture_stream_ = nullptr, saved_stream_ = nullptr;
        bool capturing_ = false;
        bool transparent_check_ = false;
        // lazily built per-level tables; guarded so that concurrent calls on different ciphertexts stay safe, as with the
        // reference's Evaluator (evaluator.h:79-87: the class holds only immutable state)
        // ciphertexts whose key-switch tail this evaluator deferred (LazyTail): completed before the evaluator goes away or starts
        // recording a graph
        friend class Ciphertext;
        void defer_tail(Ciphertext &e, uint64_t *acc, bool with_addend) const;
        void complete_tail(Ciphertext &e, LazyTail t) const;     // the plain mod-down, then the sums go back to the pool
        // deferred tensor products (LazyProduct): record / form now / take over for the fused relinearisation / discard
        bool may_defer_product(const Level &lvl, size_t batch) const;
        void defer_product(Ciphertext &dest, const Ciphertext *x, const Ciphertext *y, uint64_t *own) const;
        void complete_product(Ciphertext &dest, LazyProduct p) const;
        LazyProduct detach_product(Ciphertext &dest) const;
        void forget_product(const Ciphertext &dest, LazyProduct p) const;
        bool relinearize_from_product(Ciphertext &e, const KSwitchKeys &relin_keys) const; // false: conditions not met, nothing done
        void forget_tail(const Ciphertext &e, LazyTail t) const; // discard
        LazyTail detach_tail(Ciphertext &e) const;
        void settle_all() const;
        // mod-down by the special prime and rescale by q_last in one pass (NttTail2); e has two polynomials and a deferred tail
        void switch_key_finish_rescale(Ciphertext &e, uint64_t *acc, const Level *next, double destination_scale, bool acc_has_addend) const;
        void switch_key_finish_modswitch_bfv(Ciphertext &e, uint64_t *acc, const Level *next) const;
        mutable std::mutex lazy_mu_;
        mutable std::vector<const Ciphertext *> lazy_cts_;
        mutable std::mutex cache_mu_;
        mutable std::map<unsigned, uint32_t *> ks_maps_;
        mutable std::map<unsigned, KsTargets> ks_targets_;
        mutable unsigned *d_flag_ = nullptr;
    };
} // namespace sealhip
