// Evaluator, part 3: modulus switching / rescaling and the Galois automorphisms
#include "evaluator_common.h"
#include <atomic>

namespace sealhip
{
    // ---- modulus switching (evaluator.cpp:1201-1647)
    void Evaluator::mod_switch_scale_to_next(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        const Scheme scheme = context_.scheme();
        check_native_form(e);
        const Level &lvl = *e.level();
        const Level *next = context_.next_level(lvl);
        double destination_scale = 1.0;
        if (scheme == Scheme::ckks)
        {
            if (!scale_within_bounds(e.scale(), lvl))
                throw std::invalid_argument("scale out of bounds");
            destination_scale = e.scale() / static_cast<double>(context_.coeff_modulus()[lvl.K - 1]);
            if (!scale_within_bounds(destination_scale, *next))
                throw std::invalid_argument("scale out of bounds");
        }
        const unsigned K = lvl.K;
        const size_t N = context_.n();
        if (scheme == Scheme::ckks && e.lazy_ && e.lazy_->owner == this && e.size() == 2 && K >= 2 &&
            ntt2_supports(context_.log_n()))
        {
            // the key switch that produced e left its mod-down undone (LazyTail): both rounding divisions in one pass.  (The ring test
            // chooses the folded tail, NttBatch::tail2, which only the two-pass engine has; no route defers elsewhere.)
            const LazyTail t = detach_tail(e);
            try
            {
                switch_key_finish_rescale(e, t.acc, next, destination_scale, t.with_addend);
            }
            catch (...)
            {
                // the folded pass works in place on e's planes: after a failure they are neither the old nor the new ciphertext.
                // Leave an EMPTY object behind (size 0: every later use is rejected) rather than words that look valid
                DevicePool::global().free_words(t.acc, stream_);
                e.release();
                throw;
            }
            DevicePool::global().free_words(t.acc, stream_);
            return;
        }
        if (scheme == Scheme::bfv && e.lazy_ && e.lazy_->owner == this && e.size() == 2 && K >= 2)
        {
            // BFV: the key switch that produced e left its mod-down undone: one element-wise pass does it and this division
            const LazyTail t = detach_tail(e);
            try
            {
                switch_key_finish_modswitch_bfv(e, t.acc, next);
            }
            catch (...)
            {
                // (e's planes are untouched by the folded pass - it writes a new slab - but the sums are gone: leave an EMPTY object)
                DevicePool::global().free_words(t.acc, stream_);
                e.release();
                throw;
            }
            DevicePool::global().free_words(t.acc, stream_);
            return;
        }
        const size_t items = e.size() * e.batch();
        const unsigned n_log = (unsigned)context_.log_n();
        const ModDesc *mods = context_.dev_mods();
        size_t words = items * (K - 1) * N;
        uint64_t *out = DevicePool::global().alloc_words(words);
        try
        {
            if (scheme == Scheme::bfv)
            {
                ck(k_bfv_modswitch(mods, lvl.dev, e.data(), out, n_log, items, stream_), "bfv modswitch");
            }
            else if (scheme == Scheme::bgv)
            {
                // mod_t_and_divide_q_last_ntt_inplace (rns.cpp:1193-1236)
                const NttTables &tb = context_.ntt_tables();
                uint64_t *last = e.data() + (size_t)(K - 1) * N;
                ck(ntt_inverse(tb, plain_batch(last, (size_t)K * N, 1, (unsigned)items, K - 1), 0, stream_), "bgv modswitch intt last");
                Scratch delta(words);
                ck(k_bgv_delta(mods, host::make_mod(context_.plain_modulus()), lvl.dev.inv_q_last_mod_t, lvl.dev.q_last_mod_q, last,
                               (size_t)K * N, delta.p, n_log, K - 1, items, stream_),
                   "bgv modswitch delta");
                bgv_correct_and_combine(delta, e.data(), (size_t)K * N, lvl.dev.inv_q_last_mod_q, K - 1, items, out, nullptr,
                                        (size_t)(K - 1) * N, 1);
            }
            else
            {
                // divide_and_round_q_last_ntt_inplace (rns.cpp:830-901)
                const NttTables &tb = context_.ntt_tables();
                uint64_t *last = e.data() + (size_t)(K - 1) * N;
                ck(ntt_inverse(tb, plain_batch(last, (size_t)K * N, 1, (unsigned)items, K - 1), 0, stream_), "rescale intt last");
                ck(ntt_forward(tb,
                               plain_batch(nullptr, (size_t)(K - 1) * N, K - 1, (unsigned)items, 0)
                                   .rounded_src(last, (size_t)K * N, 1, 2, lvl.dev.half_q_last, lvl.dev.q_last, lvl.dev.round_fix)
                                   .epilogue(1, e.data(), (size_t)K * N, lvl.dev.inv_q_last_mod_q, out, nullptr, (size_t)(K - 1) * N),
                               1, stream_),
                   "rescale ntt correction + combine");
            }
        }
        catch (...)
        {
            DevicePool::global().free_words(out);
            throw;
        }
        size_t size = e.size();
        e.adopt(next, size, out, words);
        if (scheme == Scheme::ckks)
            e.scale() = destination_scale;
        else if (scheme == Scheme::bgv)
            // evaluator.cpp:1286-1292
            e.correction_factor() = host::mulmod(e.correction_factor(), lvl.dev.inv_q_last_mod_t, context_.plain_modulus());
    }

    void Evaluator::mod_switch_drop_to_next(Ciphertext &e) const
    {
        expect_scope();
        check_native_form(e);
        const Level &lvl = *e.level();
        const Level *next = context_.next_level(lvl);
        if (!scale_within_bounds(e.scale(), *next))
            throw std::invalid_argument("scale out of bounds");
        const unsigned K = lvl.K;
        const size_t items = e.size() * e.batch();
        size_t words = items * (K - 1) * context_.n();
        uint64_t *out = DevicePool::global().alloc_words(words);
        ck(k_drop_last(e.data(), out, (unsigned)context_.log_n(), K, items, stream_), "drop last");
        size_t size = e.size();
        e.adopt(next, size, out, words);
    }

    void Evaluator::mod_switch_to_next_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (e.level() == &context_.last_level())
            throw std::invalid_argument("end of modulus switching chain reached");
        switch (context_.scheme())
        {
        case Scheme::bfv:
            mod_switch_scale_to_next(e);
            break;
        case Scheme::ckks:
            mod_switch_drop_to_next(e);
            break;
        case Scheme::bgv:
            mod_switch_scale_to_next(e);
            break;
        default:
            throw std::invalid_argument("unsupported scheme");
        }
        throw_if_transparent(e);
    }

    void Evaluator::mod_switch_to_inplace(Ciphertext &e, const uint64_t *parms_id) const
    {
        StreamScope pool_scope(stream_);
        check_context(e);
        const Level *target = target_level(e.level(), parms_id);
        while (e.level() != target)
            mod_switch_to_next_inplace(e);
    }

    void Evaluator::rescale_to_next_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (e.level() == &context_.last_level())
            throw std::invalid_argument("end of modulus switching chain reached");
        switch (context_.scheme())
        {
        case Scheme::bfv:
        case Scheme::bgv:
            throw std::invalid_argument("unsupported operation for scheme type");
        case Scheme::ckks:
            mod_switch_scale_to_next(e);
            break;
        default:
            throw std::invalid_argument("unsupported scheme");
        }
        throw_if_transparent(e);
    }

    void Evaluator::rescale_to_inplace(Ciphertext &e, const uint64_t *parms_id) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        const Level *target = target_level(e.level(), parms_id);
        if (context_.scheme() != Scheme::ckks)
            throw std::invalid_argument("unsupported operation for scheme type");
        while (e.level() != target)
            mod_switch_scale_to_next(e);
        throw_if_transparent(e);
    }

    void Evaluator::mod_reduce_to_next_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (e.level() == &context_.last_level())
            throw std::invalid_argument("end of modulus switching chain reached");
        mod_switch_drop_to_next(e);
        throw_if_transparent(e);
    }

    // evaluator.cpp:1625-1647
    void Evaluator::mod_reduce_to_inplace(Ciphertext &e, const uint64_t *parms_id) const
    {
        StreamScope pool_scope(stream_);
        check_context(e);
        const Level *target = target_level(e.level(), parms_id);
        while (e.level() != target)
            mod_reduce_to_next_inplace(e);
    }

    // ---- Galois automorphisms and rotations (evaluator.cpp:2384-2559, evaluator.h:1072-1375)
    namespace
    {
        std::atomic<uint64_t> g_galois_gathered{ 0 }, g_galois_permuted{ 0 };
    }
    void galois_path_stats(uint64_t &gathered, uint64_t &permuted)
    {
        gathered = g_galois_gathered.load();
        permuted = g_galois_permuted.load();
    }
    void Evaluator::apply_galois_inplace(Ciphertext &e, uint32_t galois_elt, const KSwitchKeys &galois_keys) const
    {
        apply_galois(e, galois_elt, galois_keys, e);
    }
    // evaluator.h:1072-1087 (apply_galois): destination = encrypted; apply_galois_inplace(destination).  The permuted polynomials go
    // into a new slab either way, so the out-of-place form reads `encrypted` where it lies: no copy of the operand
    void Evaluator::apply_galois(const Ciphertext &e, uint32_t galois_elt, const KSwitchKeys &galois_keys, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        if (&dest != &e && (&dest.context() != &context_ || dest.batch() != e.batch()))
        {
            dest = e; // a destination of another shape: the reference's two steps
            return apply_galois(dest, galois_elt, galois_keys, dest);
        }
        check_valid(e, "encrypted");
        if (galois_keys.context() != &context_)
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        const Level &lvl = *e.level();
        const size_t N = context_.n();
        uint64_t m = 2 * (uint64_t)N;
        if (!(galois_elt & 1) || galois_elt >= m)
        {
            // has_key() throws invalid_argument for an even element before this check in the
            // reference (galoiskeys.h:48-57); either way the class is invalid_argument
            throw std::invalid_argument("Galois element is not valid");
        }
        if (!galois_keys.has_key(galois_index(galois_elt)))
            throw std::invalid_argument("Galois key not present");
        if (e.size() != 2)
            throw std::invalid_argument("encrypted size must be 2");
        const Scheme scheme = context_.scheme();
        check_native_form(e);

        PlaneGeom g{ (unsigned)context_.log_n(), lvl.K, (unsigned)e.batch() };
        const int ntt_form = scheme == Scheme::bfv ? 0 : 1;
        const size_t key_index = galois_index(galois_elt);
        const KsRoute route = ks_route(lvl, e.batch(), galois_keys, key_index, 0, lvl.K);
        if (route.reads_through_map())
        {
            // Round 6: batches whose key switch runs un-split with the addend folded into its sums - neither pi(c0) nor pi(c1) is ever
            // stored: the key switch's own kernels read c0 and c1 through the automorphism's index map (the opening inverse transform
            // and the diagonal terms: c1; ks2's epilogue: c0), and the result's polynomials are written by the tail alone.
            g_galois_gathered++;
            const size_t words = 2 * g.words();
            const uint64_t *c0 = e.plane(0), *c1 = e.plane(1); // (completes whatever is pending on the operand)
            uint64_t *out = DevicePool::global().alloc_words(words, stream_);
            uint64_t *old = nullptr; // in place: the operand's slab has to outlive the kernels that read it
            if (&dest == &e)
                old = dest.exchange_slab(&lvl, 2, out, words);
            else
            {
                dest.is_ntt_form() = e.is_ntt_form();
                dest.scale() = e.scale();
                dest.correction_factor() = e.correction_factor();
                dest.adopt(&lvl, 2, out, words);
            }
            try
            {
                switch_key_inplace(dest, c1, galois_keys, key_index, route, KsAddend::galois(galois_elt, c0));
                throw_if_transparent(dest);
            }
            catch (...)
            {
                if (&dest != &e)
                    dest.release(); // (as below: no half-built destination with valid-looking metadata)
                else
                {
                    // in place: the operand's words are still in `old` - give them back to the object, as the failure left nothing else
                    dest.drop_lazy();
                    DevicePool::global().free_words(dest.exchange_slab(&lvl, 2, old, words), stream_);
                }
                throw;
            }
            DevicePool::global().free_words(old, stream_);
            return;
        }
        // pi(c0) goes straight into the result slab, pi(c1) into scratch as the key-switch target, c1 starts at zero
        g_galois_permuted++;
        Scratch perm(g.words());
        const size_t words = 2 * g.words();
        uint64_t *out = DevicePool::global().alloc_words(words);
        try
        {
            ck(k_apply_galois(context_.dev_mods(), e.plane(0), out, galois_elt, ntt_form, g, 1, stream_), "apply_galois c0");
            ck(k_apply_galois(context_.dev_mods(), e.plane(1), perm.p, galois_elt, ntt_form, g, 1, stream_), "apply_galois c1");
            // (c1 = 0 is left unwritten: switch_key_inplace zeroes it only on the paths that read it, round 6)
        }
        catch (...)
        {
            DevicePool::global().free_words(out);
            throw;
        }
        if (&dest != &e)
        {
            dest.is_ntt_form() = e.is_ntt_form();
            dest.scale() = e.scale();
            dest.correction_factor() = e.correction_factor();
        }
        dest.adopt(&lvl, 2, out, words);
        try
        {
            switch_key_inplace(dest, perm.p, galois_keys, key_index, route, KsAddend::planes(true));
            throw_if_transparent(dest);
        }
        catch (...)
        {
            // a separate destination must not keep the half-built (pi(c0), 0) with valid-looking metadata: it is left
            // EMPTY - the reference leaves a copy of the operand there (evaluator.h:1130-1135: destination = encrypted first),
            // which this form never makes; in place the object is the caller's operand and stays what the failure left of it,
            // as in the reference
            if (&dest != &e)
                dest.release();
            throw;
        }
    }

    // out-of-place forms (evaluator.h:1130-1315: destination = encrypted; *_inplace(destination)): with the exact key present the
    // operand is read where it lies; the NAF fallback copies first like the reference.  The in-place forms are these with the
    // operand as destination (evaluator.h)
    void Evaluator::rotate_internal(const Ciphertext &e, int steps, const KSwitchKeys &galois_keys, Ciphertext &dest) const
    {
        expect_scope();
        if (&dest == &e)
            return rotate_internal(dest, steps, galois_keys);
        check_context(e);
        check_batching();
        if (galois_keys.context() != &context_)
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        const uint32_t elt = steps ? galois_elt_from_step(steps) : 0;
        if (steps && galois_keys.has_key(galois_index(elt)))
            return apply_galois(e, elt, galois_keys, dest);
        dest = e;
        rotate_internal(dest, steps, galois_keys);
    }
    void Evaluator::rotate_rows(const Ciphertext &e, int steps, const KSwitchKeys &gk, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        if (context_.scheme() != Scheme::bfv && context_.scheme() != Scheme::bgv)
            throw std::logic_error("unsupported scheme");
        rotate_internal(e, steps, gk, dest);
    }
    void Evaluator::rotate_vector(const Ciphertext &e, int steps, const KSwitchKeys &gk, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        if (context_.scheme() != Scheme::ckks)
            throw std::logic_error("unsupported scheme");
        rotate_internal(e, steps, gk, dest);
    }
    // (checks and forwards to apply_galois: no scope of its own)
    void Evaluator::conjugate(bool scheme_served, const Ciphertext &e, const KSwitchKeys &gk, Ciphertext &dest) const
    {
        if (!scheme_served)
            throw std::logic_error("unsupported scheme");
        check_context(e);
        check_batching();
        apply_galois(e, galois_elt_from_step(0), gk, dest);
    }
    void Evaluator::rotate_columns(const Ciphertext &e, const KSwitchKeys &gk, Ciphertext &dest) const
    {
        conjugate(context_.scheme() == Scheme::bfv || context_.scheme() == Scheme::bgv, e, gk, dest);
    }
    void Evaluator::complex_conjugate(const Ciphertext &e, const KSwitchKeys &gk, Ciphertext &dest) const
    {
        conjugate(context_.scheme() == Scheme::ckks, e, gk, dest);
    }
    void Evaluator::rotate_rows_inplace(Ciphertext &e, int steps, const KSwitchKeys &gk) const
    {
        rotate_rows(e, steps, gk, e);
    }
    void Evaluator::rotate_columns_inplace(Ciphertext &e, const KSwitchKeys &gk) const
    {
        rotate_columns(e, gk, e);
    }
    void Evaluator::rotate_vector_inplace(Ciphertext &e, int steps, const KSwitchKeys &gk) const
    {
        rotate_vector(e, steps, gk, e);
    }
    void Evaluator::complex_conjugate_inplace(Ciphertext &e, const KSwitchKeys &gk) const
    {
        complex_conjugate(e, gk, e);
    }
    // ---- Galois sets (include/sealhip.h: GaloisSet_Create, Evaluator_ApplyGaloisSet): R rotations of every item of a batch
    namespace
    {
        std::atomic<uint64_t> g_set_batched{ 0 }, g_set_looped{ 0 }, g_set_fused_launches{ 0 };
    }
    void galois_set_stats(uint64_t &batched, uint64_t &looped, uint64_t &fused_launches)
    {
        batched = g_set_batched.load();
        looped = g_set_looped.load();
        fused_launches = g_set_fused_launches.load();
    }
    void galois_set_count_fused_launch()
    {
        g_set_fused_launches++;
    }
    GaloisSet::GaloisSet(const Context &context, const KSwitchKeys &galois_keys, uint64_t count, const uint32_t *galois_elts, bool zero_is_identity)
        : ctx_(&context), keys_(&galois_keys)
    {
        if (!galois_elts)
            throw std::invalid_argument("galois_elts is null");
        if (!count || count >= (uint64_t(1) << 32))
            throw std::invalid_argument("1 <= count < 2^32");
        if (galois_keys.context() != &context)
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        const uint64_t m = 2 * (uint64_t)context.n();
        std::vector<uint64_t> host; // KsSetEntry rows: (key, element)
        std::vector<uint32_t> seen;
        for (uint64_t r = 0; r < count; r++)
        {
            const uint32_t elt = galois_elts[r];
            elts_.push_back(elt);
            if (!elt && zero_is_identity)
                continue;
            if (!(elt & 1) || elt >= m)
                throw std::invalid_argument("Galois element is not valid");
            const size_t index = Evaluator::galois_index(elt);
            if (!galois_keys.has_key(index))
                throw std::invalid_argument("Galois key not present");
            const KSwitchKeys::Key &key = galois_keys.key(index);
            register_order_ = register_order_ && key.register_order;
            entry_of_.push_back((size_t)r);
            slabs_.push_back(key.dev);
            serials_.push_back(key.serial);
            host.push_back((uint64_t)(uintptr_t)key.dev);
            host.push_back(elt);
            if (std::find(seen.begin(), seen.end(), elt) == seen.end())
                seen.push_back(elt);
        }
        distinct_ = seen.size();
        if (host.empty())
            return; // identity entries only: nothing is ever key-switched
        static_assert(sizeof(KsSetEntry) == 16, "a table row is two words");
        block_ = DevicePool::global().alloc_words(host.size());
        try
        {
            ck(hipDeviceSynchronize(), "GaloisSet upload"); // not a hot-path call: whatever used the block before is done
            copy_h2d(block_, host.data(), host.size() * 8);
        }
        catch (...)
        {
            DevicePool::global().free_words(block_);
            throw;
        }
        table_ = reinterpret_cast<const KsSetEntry *>(block_);
    }
    GaloisSet::~GaloisSet()
    {
        DevicePool::global().free_words(block_); // (ItemMap's rule: tagged by the pool, work that still reads the table is waited for by the next user)
    }
    bool GaloisSet::keys_current() const
    {
        for (size_t i = 0; i < entry_of_.size(); i++)
        {
            const size_t index = Evaluator::galois_index(elts_[entry_of_[i]]);
            if (!keys_->has_key(index) || keys_->key(index).dev != slabs_[i] || keys_->key(index).serial != serials_[i])
                return false;
        }
        return true;
    }
    bool GaloisSet::full_keys(size_t digits) const
    {
        for (size_t i = 0; i < entry_of_.size(); i++)
        {
            const KSwitchKeys::Key &key = keys_->key(Evaluator::galois_index(elts_[entry_of_[i]]));
            if (key.digit0 != 0 || key.digits < digits)
                return false;
        }
        return true;
    }

    // Item b R + r of the result = apply_galois(item b, entry r), word for word.  Where every key is in register order (N >= 2^13) the
    // B x (entries that are not the identity) rotations run as ONE key switch over that many virtual items: the route is asked with the
    // virtual batch, so the digit groups and the chunks see the real amount of work.  On its un-split folded sub-route neither pi(c0)
    // nor pi(c1) is stored - the opening inverse transform and pass 2 read the SOURCE item through the entry's index map; on the
    // others the permuted operands go to scratch by virtual item and only the key is per item.  Everything else - smaller rings, keys in
    // natural order, a digit-parallel slice of a key - is a host loop over the entries through apply_galois.
    // Identity entries are device copies on the same stream.  With none the key switch writes the destination's slab itself and may
    // leave its tail pending exactly as apply_galois does; with some it runs on the virtual batch and the items are copied into place.
    void Evaluator::apply_galois_set(const Ciphertext &e, const GaloisSet &set, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (set.context() != &context_ || set.keys().context() != &context_)
            throw std::invalid_argument("galois_set is not valid for encryption parameters");
        if (&dest == &e)
            throw std::invalid_argument("destination must be another object than encrypted");
        const size_t B = e.batch(), R = set.count(), Rn = set.switched();
        if (&dest.context() != &context_ || (uint64_t)B * R >= (uint64_t(1) << 32) || dest.batch() != B * R)
            throw std::invalid_argument("destination must be a batch of encrypted's batch times the set's count");
        if (!set.keys_current())
            throw std::invalid_argument("a Galois key was replaced after the set was made");
        if (e.size() != 2)
            throw std::invalid_argument("encrypted size must be 2");
        check_native_form(e);
        const Level &lvl = *e.level();
        const unsigned K = lvl.K;
        const size_t KN = (size_t)K * context_.n();
        const int ntt_form = context_.scheme() == Scheme::bfv ? 0 : 1;
        const KSwitchKeys &keys = set.keys();
        const uint64_t *c0 = e.plane(0), *c1 = e.plane(1); // (completes whatever is pending on the operand)
        const auto like_operand = [&](Ciphertext &c) {
            c.is_ntt_form() = e.is_ntt_form();
            c.scale() = e.scale();
            c.correction_factor() = e.correction_factor();
        };
        // item `from` of a batch of `from_batch` -> item `to` of the result's slab, both planes
        const size_t out_plane = B * R * KN, out_words = 2 * out_plane;
        const auto copy_item = [&](uint64_t *out, size_t to, const uint64_t *src, size_t from_batch, size_t from) {
            for (size_t p = 0; p < 2; p++)
                ck(hipMemcpyAsync(out + p * out_plane + to * KN, src + p * from_batch * KN + from * KN, KN * 8, hipMemcpyDeviceToDevice, stream_),
                   "galois set copy item");
        };
        const auto copy_identities = [&](uint64_t *out) {
            for (size_t b = 0; b < B; b++)
                for (size_t r = 0; r < R; r++)
                    if (!set.elt(r))
                        copy_item(out, b * R + r, c0, B, b);
        };
        const size_t V = B * Rn;
        KsRoute route;
        if (Rn)
            route = ks_route(lvl, V, keys, galois_index(set.elt(set.entry_of(0))), 0, K);
        // The set's half of the route rule (the shape's half is ks_shape_split, evaluator_keyswitch.cpp).  A set of ONE entry is the
        // single-key call on the batch: the per-item form has nothing to share there and measured behind it (C5, B = 1, R = 1: 0.343 ms
        // against 0.317 ms eager, profiles/galois_set.txt section 2, first line of the table); from two entries on the one-batch form wins
        // (R = 2: 0.478 against 0.623 / 0.570 ms) and the gap widens with R
        const bool batched = R > 1 && Rn && route.fused && set.register_order() && set.full_keys(K);
        if (R == 1 && Rn == 1)
        {
            g_set_looped++;
            return apply_galois(e, set.elt(0), keys, dest); // (same batch: the operand is read where it lies, the tail may stay pending)
        }
        if (!batched)
        {
            // the loop: one single-key call per entry over the B sources, its items copied into their places
            g_set_looped++;
            uint64_t *out = DevicePool::global().alloc_words(out_words, stream_);
            try
            {
                copy_identities(out);
                for (size_t i = 0; i < Rn; i++)
                {
                    Ciphertext one(context_, B);
                    apply_galois(e, set.elt(set.entry_of(i)), keys, one);
                    const uint64_t *words = one.plane(0); // (completes a pending tail)
                    for (size_t b = 0; b < B; b++)
                        copy_item(out, b * R + set.entry_of(i), words, B, b);
                }
            }
            catch (...)
            {
                DevicePool::global().free_words(out, stream_);
                throw;
            }
            like_operand(dest);
            dest.adopt(&lvl, 2, out, out_words);
            return;
        }
        g_set_batched++;
        const bool direct = Rn == R; // no identity entries: the virtual batch IS the result
        Ciphertext staged(context_, direct ? 1 : V);
        Ciphertext &t = direct ? dest : staged;
        const size_t t_words = 2 * V * KN;
        uint64_t *slab = DevicePool::global().alloc_words(t_words, stream_);
        like_operand(t);
        t.adopt(&lvl, 2, slab, t_words);
        try
        {
            KsSetView view;
            view.table = set.table();
            view.count = (unsigned)Rn;
            const size_t key_index = galois_index(set.elt(set.entry_of(0))); // (names a key of the set's shape; the kernels take each item's own)
            if (route.reads_through_map())
            {
                g_galois_gathered++;
                view.map = true;
                switch_key_inplace(t, c1, keys, key_index, route, KsAddend::galois_set(view, c0));
            }
            else
            {
                g_galois_permuted++;
                // pi(c0) straight into the slab, pi(c1) into scratch as the key-switch target, both by virtual item
                Scratch perm(V * KN);
                PlaneGeom g1{ (unsigned)context_.log_n(), K, 1 };
                for (size_t b = 0; b < B; b++)
                    for (size_t i = 0; i < Rn; i++)
                    {
                        const uint32_t elt = set.elt(set.entry_of(i));
                        ck(k_apply_galois(context_.dev_mods(), c0 + b * KN, slab + (b * Rn + i) * KN, elt, ntt_form, g1, 1, stream_), "galois set c0");
                        ck(k_apply_galois(context_.dev_mods(), c1 + b * KN, perm.p + (b * Rn + i) * KN, elt, ntt_form, g1, 1, stream_), "galois set c1");
                    }
                switch_key_inplace(t, perm.p, keys, key_index, route, KsAddend::planes(true).with_keys_of(view));
            }
            throw_if_transparent(t);
            if (!direct)
            {
                uint64_t *out = DevicePool::global().alloc_words(out_words, stream_);
                try
                {
                    copy_identities(out);
                    const uint64_t *words = staged.plane(0); // (completes the pending tail)
                    for (size_t b = 0; b < B; b++)
                        for (size_t i = 0; i < Rn; i++)
                            copy_item(out, b * R + set.entry_of(i), words, V, b * Rn + i);
                }
                catch (...)
                {
                    DevicePool::global().free_words(out, stream_);
                    throw;
                }
                like_operand(dest);
                dest.adopt(&lvl, 2, out, out_words);
            }
        }
        catch (...)
        {
            if (direct)
                dest.release(); // (as apply_galois: no half-built destination with valid-looking metadata)
            throw;
        }
    }

    void Evaluator::rotate_internal(Ciphertext &e, int steps, const KSwitchKeys &galois_keys) const
    {
        expect_scope();
        check_context(e);
        check_batching();
        if (galois_keys.context() != &context_)
            throw std::invalid_argument("galois_keys is not valid for encryption parameters");
        if (steps == 0)
            return;
        size_t coeff_count = context_.n();
        uint32_t elt = galois_elt_from_step(steps);
        if (galois_keys.has_key(galois_index(elt)))
        {
            apply_galois_inplace(e, elt, galois_keys);
        }
        else
        {
            std::vector<int> naf_steps = naf(steps);
            if (naf_steps.size() == 1)
                throw std::invalid_argument("Galois key not present");
            for (int step : naf_steps)
                if ((size_t)std::abs(step) != (coeff_count >> 1))
                    rotate_internal(e, step, galois_keys);
        }
    }
} // namespace sealhip
