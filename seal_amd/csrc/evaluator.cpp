// Evaluator, part 1: construction, streams and graph capture, deferred key-switch tails, negate / add / sub, transforms, plaintext operands, multiply
#include "evaluator_common.h"
#include "plain_batch_kernels.h"
#include "batch_reduce_kernels.h"
#include <atomic>

namespace sealhip
{
    // ---------------------------------------------------------------- Evaluator
    Evaluator::Evaluator(const Context &context) : context_(context)
    {
        void *p = nullptr;
        ck(hipMalloc(&p, sizeof(unsigned)), "hipMalloc flag");
        d_flag_ = (unsigned *)p;
    }
    // ---- deferred key-switch tails (LazyTail, evaluator.h)
    std::atomic<uint64_t> g_tail_folded{ 0 }, g_tail_plain{ 0 }, g_tail_dropped{ 0 };
    void lazy_tail_stats(uint64_t &folded, uint64_t &plain, uint64_t &dropped)
    {
        folded = g_tail_folded.load();
        plain = g_tail_plain.load();
        dropped = g_tail_dropped.load();
    }
    void Evaluator::defer_tail(Ciphertext &e, uint64_t *acc, bool with_addend) const
    {
        e.lazy_ = new LazyTail{ this, acc, with_addend };
        std::lock_guard<std::mutex> lock(lazy_mu_);
        lazy_cts_.push_back(&e);
    }
    LazyTail Evaluator::detach_tail(Ciphertext &e) const
    {
        const LazyTail t = *e.lazy_;
        delete e.lazy_;
        e.lazy_ = nullptr;
        std::lock_guard<std::mutex> lock(lazy_mu_);
        lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &e), lazy_cts_.end());
        return t;
    }
    void Evaluator::forget_tail(const Ciphertext &e, LazyTail t) const
    {
        StreamScope pool_scope(stream_);
        {
            std::lock_guard<std::mutex> lock(lazy_mu_);
            lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &e), lazy_cts_.end());
        }
        DevicePool::global().free_words(t.acc, stream_);
        g_tail_dropped++;
    }
    void Evaluator::complete_tail(Ciphertext &e, LazyTail t) const
    {
        const hipStream_t caller = DevicePool::thread_stream(); // (read before this call's own scope replaces it)
        StreamScope pool_scope(stream_);
        {
            std::lock_guard<std::mutex> lock(lazy_mu_);
            lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &e), lazy_cts_.end());
        }
        // the sums were produced on this evaluator's stream: the tail runs there too; a caller working on another stream
        // (another evaluator, a host copy) continues only when it is done
        if (ks_switches().trace) // tests: which tail ran
            std::fprintf(stderr, t.with_addend ? "[ks] plain tail, addend in the sums\n" : "[ks] plain tail\n");
        g_tail_plain++;
        try
        {
            switch_key_finish(e, t.acc, 1, t.with_addend);
        }
        catch (...)
        {
            DevicePool::global().free_words(t.acc, stream_);
            throw;
        }
        DevicePool::global().free_words(t.acc, stream_);
        if (caller != stream_ && !capturing_) // (a stream that is recording cannot be waited for: its work runs when the graph does)
            ck(hipStreamSynchronize(stream_), "deferred key-switch tail");
    }
    // ---- deferred tensor products (evaluator.h: LazyProduct)
    namespace
    {
        std::atomic<uint64_t> g_prod_fused{ 0 }, g_prod_formed{ 0 }, g_prod_dropped{ 0 };
    }
    void lazy_product_stats(uint64_t &fused, uint64_t &formed, uint64_t &dropped)
    {
        fused = g_prod_fused.load();
        formed = g_prod_formed.load();
        dropped = g_prod_dropped.load();
    }
    // CKKS at a two-pass size (ntt2_supports chooses whether a product may stay pending: only that engine forms it while loading,
    // NttBatch::prod_x), a batch whose key switch runs un-split - the shape's half of the route's rule, no key being known yet.
    // SEALHIP_LAZY_PRODUCT_MIN_WGS moves that rule's threshold (1024 pass-2 workgroups): tests reach the fused path at small batches with it and SEALHIP_KS_SPLIT=1
    bool Evaluator::may_defer_product(const Level &lvl, size_t batch) const
    {
        if (!KsSwitches::lazy_product() || capturing_ || transparent_check_ || lvl.K < 2 || !ntt2_supports(context_.log_n()))
            return false;
        size_t min_wgs;
        if (KsSwitches::lazy_product_min_wgs(min_wgs))
            return batch * (lvl.K + 1) * (context_.n() >> 12) > min_wgs;
        return ks_shape_split(lvl, batch) <= 1;
    }
    void Evaluator::defer_product(Ciphertext &dest, const Ciphertext *x, const Ciphertext *y, uint64_t *own) const
    {
        dest.lazy_prod_ = new LazyProduct{ this, x, y, own };
        lazy_product_link(&dest, *dest.lazy_prod_);
        std::lock_guard<std::mutex> lock(lazy_mu_);
        lazy_cts_.push_back(&dest);
    }
    // (called by Ciphertext::settle_product, which unlinks the operands and deletes the record afterwards)
    void Evaluator::complete_product(Ciphertext &dest, LazyProduct p) const
    {
        const hipStream_t caller = DevicePool::thread_stream();
        StreamScope pool_scope(stream_);
        {
            std::lock_guard<std::mutex> lock(lazy_mu_);
            lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &dest), lazy_cts_.end());
        }
        const Level &lvl = *dest.level_;
        PlaneGeom g{ (unsigned)context_.log_n(), lvl.K, (unsigned)dest.batch() };
        g_prod_formed++;
        hipError_t err = hipSuccess;
        try
        {
            err = k_ckks_multiply_2x2(context_.dev_mods(), context_.ntt_tables().fpd, nullptr, p.xw(), p.yw(), dest.data_, g, stream_);
        }
        catch (...)
        {
            DevicePool::global().free_words(p.own, stream_);
            throw;
        }
        DevicePool::global().free_words(p.own, stream_); // (an in-place product's previous slab: read by the kernel just queued on this stream)
        ck(err, "ckks_multiply (deferred)");
        // the product is formed on this evaluator's stream; a caller on another stream - the one about to read the words or to
        // overwrite an operand - continues only when it is done
        if (caller != stream_ && !capturing_)
            ck(hipStreamSynchronize(stream_), "deferred tensor product");
    }
    // the fused relinearisation takes the record over: the destination is no longer pending, the live operands are released (an owned
    // slab is now the caller's to free)
    LazyProduct Evaluator::detach_product(Ciphertext &dest) const
    {
        const LazyProduct p = *dest.lazy_prod_;
        delete dest.lazy_prod_;
        dest.lazy_prod_ = nullptr;
        lazy_product_unlink(&dest, p);
        std::lock_guard<std::mutex> lock(lazy_mu_);
        lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &dest), lazy_cts_.end());
        return p;
    }
    void Evaluator::forget_product(const Ciphertext &dest, LazyProduct p) const
    {
        StreamScope pool_scope(stream_);
        {
            std::lock_guard<std::mutex> lock(lazy_mu_);
            lazy_cts_.erase(std::remove(lazy_cts_.begin(), lazy_cts_.end(), &dest), lazy_cts_.end());
        }
        DevicePool::global().free_words(p.own, stream_);
        g_prod_dropped++;
    }
    void lazy_product_count_fused()
    {
        g_prod_fused++;
    }

    void Evaluator::settle_all() const
    {
        for (;;)
        {
            const Ciphertext *c = nullptr;
            {
                std::lock_guard<std::mutex> lock(lazy_mu_);
                if (lazy_cts_.empty())
                    return;
                c = lazy_cts_.back();
            }
            c->settle(); // removes it from the list
        }
    }

    Evaluator::~Evaluator()
    {
        try
        {
            settle_all();
        }
        catch (...)
        {
            // a tail could not be completed (device error): no ciphertext may keep a LazyTail whose owner is gone - the pending
            // sums are discarded, the objects stay what they were before their key switch's mod-down (their next use is still
            // memory-safe; the device error itself is what the caller sees on its next call)
            for (;;)
            {
                const Ciphertext *c = nullptr;
                {
                    std::lock_guard<std::mutex> lock(lazy_mu_);
                    if (lazy_cts_.empty())
                        break;
                    c = lazy_cts_.back();
                }
                const_cast<Ciphertext *>(c)->drop_product(); // either removes it from the list
                const_cast<Ciphertext *>(c)->drop_lazy();
            }
        }
        for (auto &kv : ks_maps_)
            (void)hipFree(kv.second);
        for (auto &kv : ks_targets_)
            (void)hipFree(kv.second.dev);
        if (d_flag_)
            (void)hipFree(d_flag_);
        if (capture_stream_)
            (void)hipStreamDestroy(capture_stream_);
        DevicePool::global().unregister_stream(capturing_ ? saved_stream_ : stream_);
    }
    void Evaluator::set_stream(hipStream_t s)
    {
        if (capturing_)
            throw std::logic_error("a capture is in progress");
        if (s == stream_)
            return;
        settle_all(); // deferred tails belong to the stream their sums were produced on
        DevicePool::global().unregister_stream(stream_);
        stream_ = s;
        DevicePool::global().register_stream(stream_);
    }
    Evaluator::Graph::~Graph()
    {
        if (exec)
            (void)hipGraphExecDestroy(exec);
        DevicePool::global().release_held(scratch);
    }
    void Evaluator::begin_capture()
    {
        if (capturing_)
            throw std::logic_error("a capture is already in progress");
        if (transparent_check_)
            throw std::logic_error("the transparent-ciphertext check reads device memory back and cannot be captured");
        settle_all(); // deferred tails hold pool blocks of their own: complete them before the recording starts
        if (!capture_stream_)
            ck(hipStreamCreateWithFlags(&capture_stream_, hipStreamNonBlocking), "capture stream");
        // drain the device: every cached pool block is idle from here on, and the recording takes its scratch only from
        // idle or fresh blocks, which then belong to the graph (pool.h)
        ck(hipDeviceSynchronize(), "device synchronize");
        saved_stream_ = stream_;
        stream_ = capture_stream_;
        // relaxed: a pool miss may still hipMalloc while recording (it touches no stream)
        hipError_t e = hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed);
        if (e != hipSuccess)
        {
            stream_ = saved_stream_;
            ck(e, "hipStreamBeginCapture");
        }
        DevicePool::global().begin_hold();
        capturing_ = true;
    }
    Evaluator::Graph *Evaluator::end_capture()
    {
        if (!capturing_)
            throw std::logic_error("no capture in progress");
        // a tail deferred inside the recording and not consumed by it runs as the recording's last work (on the capture stream)
        try
        {
            settle_all();
        }
        catch (...)
        {
            hipGraph_t dead = nullptr;
            (void)hipStreamEndCapture(stream_, &dead);
            if (dead)
                (void)hipGraphDestroy(dead);
            stream_ = saved_stream_;
            capturing_ = false;
            DevicePool::global().release_held(DevicePool::global().end_hold());
            throw;
        }
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamEndCapture(stream_, &graph);
        stream_ = saved_stream_;
        capturing_ = false;
        std::unique_ptr<Graph> g(new Graph);
        g->scratch = DevicePool::global().end_hold();
        ck(e, "hipStreamEndCapture");
        e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        ck(e, "hipGraphInstantiate");
        return g.release();
    }
    void Evaluator::launch_graph(const Graph *graph) const
    {
        if (capturing_)
            throw std::logic_error("a capture is in progress");
        if (!graph || !graph->exec)
            throw std::invalid_argument("graph");
        ck(hipGraphLaunch(graph->exec, stream_), "hipGraphLaunch");
    }

    void Evaluator::synchronize() const
    {
        ck(hipStreamSynchronize(stream_), "stream synchronize");
    }

    size_t Evaluator::relin_index(size_t key_power)
    {
        if (key_power < 2)
            throw std::invalid_argument("key_power cannot be less than 2");
        return key_power - 2;
    }
    size_t Evaluator::galois_index(uint32_t galois_elt)
    {
        if (!(galois_elt & 1))
            throw std::invalid_argument("galois_elt is not valid");
        return (galois_elt - 1) >> 1;
    }
    uint32_t Evaluator::galois_elt_from_step(int step) const
    {
        // GaloisTool::get_elt_from_step (util/galois.cpp:53-95), generator 3
        uint32_t n = (uint32_t)context_.n();
        uint32_t m32 = n * 2;
        uint64_t m = m32;
        if (step == 0)
            return (uint32_t)(m - 1);
        bool sign = step < 0;
        uint32_t pos_step = (uint32_t)std::abs(step);
        if (pos_step >= (n >> 1))
            throw std::invalid_argument("step count too large");
        pos_step &= m32 - 1;
        int s = sign ? (int)(n >> 1) - (int)pos_step : (int)pos_step;
        uint64_t elt = 1;
        while (s--)
        {
            elt *= 3;
            elt &= m - 1;
        }
        return (uint32_t)elt;
    }

    const uint32_t *Evaluator::ks_comp_prime(unsigned K) const
    {
        std::lock_guard<std::mutex> g(cache_mu_);
        auto it = ks_maps_.find(K);
        if (it != ks_maps_.end())
            return it->second;
        // [ (I*K + J) -> prime(I) for I in 0..K ] followed by [ i -> prime(i) for i in 0..K ]
        unsigned L = context_.key_level().K;
        std::vector<uint32_t> m;
        for (unsigned I = 0; I <= K; I++)
            for (unsigned J = 0; J < K; J++)
                m.push_back(I == K ? L - 1 : I);
        for (unsigned I = 0; I <= K; I++)
            m.push_back(I == K ? L - 1 : I);
        void *p = nullptr;
        ck(hipMalloc(&p, m.size() * 4), "hipMalloc ks map");
        ck(hipMemcpy(p, m.data(), m.size() * 4, hipMemcpyHostToDevice), "upload ks map");
        ks_maps_[K] = (uint32_t *)p;
        return (uint32_t *)p;
    }

    const Evaluator::KsTargets &Evaluator::ks_targets(unsigned K) const
    {
        std::lock_guard<std::mutex> g(cache_mu_);
        auto it = ks_targets_.find(K);
        if (it != ks_targets_.end())
            return it->second;
        // target moduli of a key switch at a level with K data primes: q_0..q_{K-1} and the special
        // prime (slot I = K, pool prime and key component L-1), split by arithmetic back end
        const unsigned L = context_.key_level().K;
        std::vector<uint32_t> t1[2], t2[2];
        for (unsigned I = 0; I <= K; I++)
        {
            const unsigned prime = I == K ? L - 1 : I;
            const int fp = context_.fp_prime(prime) ? 1 : 0;
            t1[fp].push_back(I);
            t1[fp].push_back(prime);
            t2[fp].push_back(I);
            t2[fp].push_back(prime);
            t2[fp].push_back(prime);
            t2[fp].push_back(key_comp_offset_units(context_.ntt_tables(), prime)); // where the component sits inside a digit (ntt2_kernels.h)
        }
        KsTargets kt;
        kt.n_int = (unsigned)t1[0].size() / 2;
        kt.n_fp = (unsigned)t1[1].size() / 2;
        // [targets1: int..., fp...][targets2: int..., fp...]
        std::vector<uint32_t> all;
        for (int fp = 0; fp < 2; fp++)
            all.insert(all.end(), t1[fp].begin(), t1[fp].end());
        for (int fp = 0; fp < 2; fp++)
            all.insert(all.end(), t2[fp].begin(), t2[fp].end());
        void *p = nullptr;
        ck(hipMalloc(&p, all.size() * 4 + 4), "hipMalloc ks targets");
        ck(hipMemcpy(p, all.data(), all.size() * 4, hipMemcpyHostToDevice), "upload ks targets");
        kt.dev = (uint32_t *)p;
        return ks_targets_[K] = kt;
    }

    // arithmetic class of the K data primes and the special prime together (NttBatch::cls_hint for batches that name them through
    // ks_comp_prime's map): 0 all on the integer back end, 1 all on the double-precision one, -1 mixed
    int Evaluator::ks_class_hint(unsigned K) const
    {
        const unsigned L = context_.key_level().K;
        unsigned fp = context_.fp_prime(L - 1) ? 1 : 0;
        for (unsigned i = 0; i < K; i++)
            fp += context_.fp_prime(i) ? 1 : 0;
        return fp == 0 ? 0 : (fp == K + 1 ? 1 : -1);
    }

    bool Evaluator::scale_within_bounds(double scale, const Level &lvl) const
    {
        // is_scale_within_bounds (evaluator.cpp:29-48)
        int bound = 0;
        switch (context_.scheme())
        {
        case Scheme::bfv:
        case Scheme::bgv:
            bound = host::bit_count(context_.plain_modulus());
            break;
        case Scheme::ckks:
            bound = lvl.total_coeff_modulus_bit_count;
            break;
        default:
            bound = -1;
        }
        return !(!std::isnormal(scale) || scale <= 0 || (static_cast<int>(std::log2(scale)) >= bound));
    }

    void Evaluator::check_native_form(const Ciphertext &e) const
    {
        const Scheme scheme = context_.scheme();
        if (scheme == Scheme::bfv && e.is_ntt_form())
            throw std::invalid_argument("BFV encrypted cannot be in NTT form");
        if (scheme == Scheme::ckks && !e.is_ntt_form())
            throw std::invalid_argument("CKKS encrypted must be in NTT form");
        if (scheme == Scheme::bgv && !e.is_ntt_form())
            throw std::invalid_argument("BGV encrypted must be in NTT form");
    }
    void Evaluator::check_valid(const Ciphertext &ct, const char *what) const
    {
        // is_metadata_valid_for + is_buffer_valid (valcheck.cpp:81-139, 221-237)
        bool ok = &ct.context() == &context_ && ct.level() != nullptr;
        if (ok)
        {
            const Level &l = *ct.level();
            ok = l.chain_index <= context_.first_level().chain_index;
            size_t size = ct.size();
            ok = ok && !((size < 2 && size != 0) || size > 16);
            double scale = ct.scale();
            Scheme s = context_.scheme();
            if (s == Scheme::bfv || s == Scheme::bgv)
                ok = ok && scale == 1.0;
            else
                ok = ok && (std::isnormal(scale) && scale > 0);
            uint64_t cf = ct.correction_factor();
            if (s == Scheme::bgv)
                ok = ok && !(cf == 0 || cf >= context_.plain_modulus());
            else
                ok = ok && cf == 1;
            ok = ok && (ct.word_count() == 0 || ct.has_storage());
            ok = ok && ct.word_count() <= ct.capacity_words(); // is_buffer_valid (valcheck.cpp:172-198): size x K x N words are there
        }
        if (!ok)
            throw std::invalid_argument(std::string(what) + " is not valid for encryption parameters");
    }

    void Evaluator::check_context(const Ciphertext &ct, const char *what) const
    {
        if (&ct.context() != &context_ || !ct.level())
            throw std::invalid_argument(std::string(what) + " is not valid for encryption parameters");
    }
    void Evaluator::check_batching() const
    {
        if (!context_.using_batching())
            throw std::logic_error("encryption parameters do not support batching");
    }
    const Level *Evaluator::target_level(const Level *level, const uint64_t *parms_id) const
    {
        const Level *target = context_.level_by_parms_id(parms_id);
        if (!target)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        if (level->chain_index < target->chain_index)
            throw std::invalid_argument("cannot switch to higher level modulus");
        return target;
    }
    // rows x inner times inner x cols: every dimension and every product of two fits 32 bits (the tiled products' index arithmetic)
    void Evaluator::check_matmul_shape(size_t rows, size_t inner, size_t cols) const
    {
        if (!rows || !inner || !cols || (rows >> 32) || (inner >> 32) || (cols >> 32) || ((rows * inner) >> 32) || ((inner * cols) >> 32) ||
            ((rows * cols) >> 32))
            throw std::invalid_argument("1 <= rows, inner, cols and rows * inner, inner * cols, rows * cols < 2^32");
    }

    bool Evaluator::is_transparent(const Ciphertext &ct) const
    {
        // Ciphertext::is_transparent (ciphertext.h:451-456)
        StreamScope pool_scope(stream_); // (public, and Ciphertext_IsTransparent calls it on an evaluator of its own)
        if (!ct.word_count() || ct.size() < 2)
            return true;
        Scratch word(1); // per call: concurrent checks on different ciphertexts must not share the flag
        unsigned *d_flag = reinterpret_cast<unsigned *>(word.p);
        unsigned zero = 0;
        ck(hipMemcpyAsync(d_flag, &zero, sizeof(zero), hipMemcpyHostToDevice, stream_), "flag reset");
        ck(k_any_nonzero(ct.plane(1), (ct.size() - 1) * ct.plane_words(), d_flag, stream_), "any_nonzero");
        unsigned flag = 0;
        ck(hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, stream_), "flag read");
        ck(hipStreamSynchronize(stream_), "flag sync");
        return flag == 0;
    }
    void Evaluator::throw_if_transparent(const Ciphertext &ct) const
    {
        expect_scope();
        if (transparent_check_ && is_transparent(ct))
            throw std::logic_error("result ciphertext is transparent");
    }

    // ---- negate / add / sub (evaluator.cpp:130-350)
    void Evaluator::negate_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        PlaneGeom g{ (unsigned)context_.log_n(), e.level()->K, (unsigned)e.batch() };
        if (e.size())
            ck(k_addsub(context_.dev_mods(), e.data(), nullptr, e.data(), 2, g, (unsigned)e.size(), stream_), "negate");
        throw_if_transparent(e);
    }

    void Evaluator::add_inplace(Ciphertext &e1, const Ciphertext &e2) const
    {
        StreamScope pool_scope(stream_);
        addsub(e1, e2, 0);
    }
    void Evaluator::sub_inplace(Ciphertext &e1, const Ciphertext &e2) const
    {
        StreamScope pool_scope(stream_);
        addsub(e1, e2, 1);
    }
    // e1 <- e1 + e2 (op 0) or e1 - e2 (op 1); where e2 is the longer one its tail is copied or negated
    void Evaluator::addsub(Ciphertext &e1, const Ciphertext &e2, int op) const
    {
        expect_scope();
        check_valid(e1, "encrypted1");
        check_valid(e2, "encrypted2");
        if (e1.level() != e2.level())
            throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        if (e1.is_ntt_form() != e2.is_ntt_form())
            throw std::invalid_argument("NTT form mismatch");
        if (!are_close(e1.scale(), e2.scale()))
            throw std::invalid_argument("scale mismatch");
        if (e1.batch() != e2.batch())
            throw std::invalid_argument("batch mismatch");
        if (e1.correction_factor() != e2.correction_factor())
        {
            // balance the correction factors and scale both operands first (BGV, evaluator.cpp:173-192, 259-278)
            uint64_t f, m1, m2;
            balance_correction_factors(e1.correction_factor(), e2.correction_factor(), context_.plain_modulus(), f, m1, m2);
            PlaneGeom gg{ (unsigned)context_.log_n(), e1.level()->K, (unsigned)e1.batch() };
            if (e1.size())
                ck(k_mul_scalar(context_.dev_mods(), e1.data(), e1.data(), m1, gg, (unsigned)e1.size(), stream_),
                   op ? "sub: scale encrypted1" : "add: scale encrypted1");
            Ciphertext copy(e2);
            if (copy.size())
                ck(k_mul_scalar(context_.dev_mods(), copy.data(), copy.data(), m2, gg, (unsigned)copy.size(), stream_),
                   op ? "sub: scale encrypted2" : "add: scale encrypted2");
            e1.correction_factor() = f;
            copy.correction_factor() = f;
            addsub(e1, copy, op);
            return;
        }
        size_t s1 = e1.size(), s2 = e2.size();
        size_t mx = std::max(s1, s2), mn = std::min(s1, s2);
        e1.resize(e1.level(), mx, stream_);
        PlaneGeom g{ (unsigned)context_.log_n(), e1.level()->K, (unsigned)e1.batch() };
        if (mn)
            ck(k_addsub(context_.dev_mods(), e1.data(), e2.data(), e1.data(), op, g, (unsigned)mn, stream_), op ? "sub" : "add");
        if (s1 < s2 && op == 0)
            ck(hipMemcpyAsync(e1.plane(s1), e2.plane(mn), (s2 - s1) * e1.plane_words() * 8, hipMemcpyDeviceToDevice, stream_),
               "add copy tail");
        else if (s1 < s2)
            ck(k_addsub(context_.dev_mods(), e2.plane(mn), nullptr, e1.plane(mn), 2, g, (unsigned)(s2 - mn), stream_), "sub negate tail");
        throw_if_transparent(e1);
    }

    // ---- transforms (evaluator.cpp:2289-2382)
    void Evaluator::transform_to_ntt_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (e.is_ntt_form())
            throw std::invalid_argument("encrypted is already in NTT form");
        unsigned K = e.level()->K;
        NttBatch b = plain_batch(e.data(), (size_t)K * context_.n(), K, (unsigned)(e.size() * e.batch()), 0);
        ck(ntt_forward(context_.ntt_tables(), b, 0, stream_), "ntt_forward");
        e.is_ntt_form() = true;
        throw_if_transparent(e);
    }
    void Evaluator::transform_from_ntt_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        if (!e.is_ntt_form())
            throw std::invalid_argument("encrypted_ntt is not in NTT form");
        unsigned K = e.level()->K;
        NttBatch b = plain_batch(e.data(), (size_t)K * context_.n(), K, (unsigned)(e.size() * e.batch()), 0);
        ck(ntt_inverse(context_.ntt_tables(), b, 0, stream_), "ntt_inverse");
        e.is_ntt_form() = false;
        throw_if_transparent(e);
    }

    // ---- plaintext operands (evaluator.cpp:1760-2287) and many-operand forms (242-261, 1649-1757)
    void Evaluator::check_valid(const Plaintext &p) const
    {
        // is_metadata_valid_for(Plaintext) + is_buffer_valid (valcheck.cpp:28-79, 209-219)
        bool ok = &p.context() == &context_;
        if (ok && p.is_ntt_form())
        {
            const Level &l = *p.level();
            ok = l.chain_index <= context_.first_level().chain_index && p.coeff_count() == (size_t)l.K * context_.n();
        }
        else if (ok)
            ok = p.coeff_count() <= context_.n();
        if (ok && context_.scheme() == Scheme::ckks)
            ok = std::isnormal(p.scale()) && p.scale() > 0;
        ok = ok && (p.coeff_count() == 0 || p.data() != nullptr);
        if (!ok)
            throw std::invalid_argument("plain is not valid for encryption parameters");
    }

    // ---- plaintext operands.  One code path serves a Plaintext handle (one plaintext for every item of the batch) and raw device
    // words with one plaintext per item (include/sealhip.h: Evaluator_AddPlainDevice ...): the shared plaintext is the per-item one
    // whose item stride is zero (plain_batch_kernels.h).
    struct Evaluator::PlainOperand
    {
        const uint64_t *words;
        size_t stride;      // words from one item's plaintext to the next; 0 = one plaintext shared by every item
        size_t coeff_count; // coefficient form: the words one plaintext holds (<= N)
        bool ntt;
        const Level *level; // of the words in NTT form; per item: the ciphertext's
        double scale;
        PlainOperand(const Plaintext &p)
            : words(p.data()), stride(0), coeff_count(p.coeff_count()), ntt(p.is_ntt_form()), level(p.level()), scale(p.scale())
        {
        }
        // one plaintext per item of a batch: [batch][N] coefficients, or [batch][K][N] words at lvl (BFV / BGV plaintexts have scale 1)
        PlainOperand(const Context &ctx, const Level *lvl, const uint64_t *plain, bool plain_is_ntt, double plain_scale)
            : words(plain), stride(plain_is_ntt ? lvl->K * ctx.n() : ctx.n()), coeff_count(ctx.n()), ntt(plain_is_ntt), level(lvl),
              scale(ctx.scheme() == Scheme::ckks ? plain_scale : 1.0)
        {
        }
    };
    namespace
    {
        constexpr size_t kPlainBatchScratchBytes = size_t(256) << 20; // per chunk of lifted plaintexts (include/sealhip.h)
        // items whose lifted plaintexts [K][N] fit the scratch of one chunk
        size_t plain_chunk_items(size_t item_words)
        {
            size_t budget = kPlainBatchScratchBytes;
            if (const char *e = shl_ab_getenv("SEALHIP_PLAIN_SCRATCH_BYTES")) // development builds only: chunk edges at small N
                budget = (size_t)std::strtoull(e, nullptr, 10);
            return std::max<size_t>(1, budget / (item_words * 8));
        }
        // qualifiers.using_fast_plain_lift: t smaller than every prime of the level
        bool fast_plain_lift(const Context &ctx, const Level &lvl)
        {
            bool fast = true;
            for (unsigned i = 0; i < lvl.K; i++)
                fast = fast && ctx.plain_modulus() < ctx.coeff_modulus()[i];
            return fast;
        }
    } // namespace

    // Coefficient-form plaintexts -> NTT-form words [K][N] at lvl (the centred lift of evaluator.cpp:2098-2125, 2243-2282, times
    // scale_by modulo t, then the forward transform), a chunk at a time: use(b0, items, lifted, stride) applies the chunk to the
    // `items` ciphertext items from b0 on, item b with the words at lifted + (b - b0) * stride.  A shared plaintext is one chunk of
    // one plaintext for all `batch` items (stride 0).  out: where the words go instead of a chunk's scratch - all of them at once.
    template <class Use>
    void Evaluator::lift_chunks(const PlainOperand &plain, const Level &lvl, uint64_t scale_by, size_t batch, uint64_t *out, Use use) const
    {
        const size_t words = (size_t)lvl.K * context_.n(), count = plain.stride ? batch : 1;
        const size_t chunk = out ? count : std::min(plain_chunk_items(words), count);
        std::unique_ptr<Scratch> scratch(out ? nullptr : new Scratch(chunk * words));
        uint64_t *lifted = out ? out : scratch->p;
        for (size_t b0 = 0; b0 < count; b0 += chunk)
        {
            const unsigned items = (unsigned)std::min(chunk, count - b0);
            ck(k_plain_lift_batch(context_.dev_mods(), host::make_mod(context_.plain_modulus()), scale_by, plain.words + b0 * plain.stride,
                                  plain.stride, plain.coeff_count, lvl.dev.plain_upper_half_threshold, lvl.dev.upper_half_inc, lifted,
                                  (unsigned)context_.log_n(), lvl.K, items, stream_),
               "plain lift");
            ck(ntt_forward(context_.ntt_tables(), plain_batch(lifted, words, lvl.K, items, 0), 0, stream_), "plain ntt");
            if (plain.stride)
                use(b0, items, lifted, words);
            else
                use(0, (unsigned)batch, lifted, 0);
        }
    }

    void Evaluator::transform_to_ntt_inplace(Plaintext &plain, const uint64_t *parms_id) const
    {
        StreamScope pool_scope(stream_);
        check_valid(plain);
        const Level *lvl = context_.level_by_parms_id(parms_id);
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for the current context");
        if (plain.is_ntt_form())
            throw std::invalid_argument("plain is already in NTT form");
        if (context_.scheme() == Scheme::ckks)
            throw std::invalid_argument("CKKS plain must be in NTT form");
        const size_t words = (size_t)lvl->K * context_.n();
        uint64_t *out = DevicePool::global().alloc_words(words);
        try
        {
            lift_chunks(plain, *lvl, 1, 1, out, [](size_t, unsigned, const uint64_t *, size_t) {});
        }
        catch (...)
        {
            DevicePool::global().free_words(out);
            throw;
        }
        plain.adopt(out, words, words);
        plain.set_level(lvl);
    }

    void Evaluator::mod_switch_to_next_inplace(Plaintext &plain) const
    {
        StreamScope pool_scope(stream_);
        // mod_switch_drop_to_next(Plaintext) (evaluator.cpp:1369-1402): the flat [K][N] array keeps its first K-1 components
        check_valid(plain);
        if (!plain.is_ntt_form())
            throw std::invalid_argument("plain is not in NTT form");
        const Level *next = context_.next_level(*plain.level());
        if (!next)
            throw std::invalid_argument("end of modulus switching chain reached");
        if (!scale_within_bounds(plain.scale(), *next))
            throw std::invalid_argument("scale out of bounds");
        plain.adopt_count((size_t)next->K * context_.n());
        plain.set_level(next);
    }
    void Evaluator::mod_switch_to_inplace(Plaintext &plain, const uint64_t *parms_id) const
    {
        StreamScope pool_scope(stream_);
        check_valid(plain);
        if (!plain.is_ntt_form())
            throw std::invalid_argument("plain is not in NTT form");
        const Level *target = target_level(plain.level(), parms_id);
        while (plain.level() != target)
            mod_switch_to_next_inplace(plain);
    }

    void Evaluator::add_plain_inplace(Ciphertext &e, const Plaintext &plain) const
    {
        StreamScope pool_scope(stream_);
        // add_plain_inplace / sub_plain_inplace share everything but the sign
        check_valid(e, "encrypted");
        check_valid(plain);
        addsub_plain(e, plain, 0, e);
    }
    void Evaluator::sub_plain_inplace(Ciphertext &e, const Plaintext &plain) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        check_valid(plain);
        addsub_plain(e, plain, 1, e);
    }
    void Evaluator::multiply_plain_inplace(Ciphertext &e, const Plaintext &plain) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        check_valid(plain);
        multiply_plain(e, plain, e);
    }
    void Evaluator::check_addsub_plain_forms(const Ciphertext &e, bool plain_is_ntt, const Level *plain_level, double plain_scale) const
    {
        const Scheme scheme = context_.scheme();
        if (scheme == Scheme::bfv)
        {
            if (e.is_ntt_form())
                throw std::invalid_argument("BFV encrypted cannot be in NTT form");
            if (plain_is_ntt)
                throw std::invalid_argument("BFV plain cannot be in NTT form");
        }
        else if (scheme == Scheme::ckks)
        {
            if (!e.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form");
            if (!plain_is_ntt)
                throw std::invalid_argument("CKKS plain must be in NTT form");
            if (e.level() != plain_level)
                throw std::invalid_argument("encrypted and plain parameter mismatch");
            if (!are_close(e.scale(), plain_scale))
                throw std::invalid_argument("scale mismatch");
        }
        else
        {
            if (!e.is_ntt_form())
                throw std::invalid_argument("BGV encrypted must be in NTT form");
            if (plain_is_ntt)
                throw std::invalid_argument("BGV plain cannot be in NTT form");
        }
        if (e.size() < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
    }
    void Evaluator::check_plain_device(const Ciphertext &e, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                       const Ciphertext &dest, bool per_item, size_t scalar_rows, bool narrow_scalars) const
    {
        const std::string name = scalar_rows ? "device_scalars" : "device_plain";
        check_valid(e, "encrypted");
        if (!plain)
            throw std::invalid_argument(name + " is null");
        if ((uintptr_t)plain % 16)
            throw std::invalid_argument(name + " must be 16-byte aligned");
        if (!batch || (per_item && batch != e.batch()))
            throw std::invalid_argument("batch does not equal the ciphertext's batch");
        if (context_.scheme() == Scheme::ckks)
        {
            if (!plain_is_ntt)
                throw std::invalid_argument("CKKS plain must be in NTT form");
            if (!std::isnormal(scale) || scale <= 0) // is_metadata_valid_for(Plaintext)
                throw std::invalid_argument("plain is not valid for encryption parameters");
        }
        // a plaintext is [K][N] words or [N] coefficients; a scalar is [K] words or one 32-bit integer, scalar_rows rows of `batch` of them
        const size_t plain_bytes = scalar_rows ? scalar_rows * batch * (narrow_scalars ? 4 : e.level()->K * 8)
                                               : batch * (plain_is_ntt ? (size_t)e.level()->K * context_.n() : context_.n()) * 8;
        if (e.has_storage() && words_overlap(plain, plain_bytes, e.data(), e.capacity_words() * 8))
            throw std::invalid_argument(name + " and encrypted overlap");
        if (&dest != &e && dest.has_storage() && words_overlap(plain, plain_bytes, dest.data_, dest.capacity_words() * 8))
            throw std::invalid_argument(name + " and destination overlap");
    }
    uint64_t *Evaluator::begin_result(const Ciphertext &e, Ciphertext &dest) const
    {
        if (&dest == &e)
            return dest.data();
        e.settle(); // the operand's words are read by what follows
        if (dest.ctx_ != e.ctx_ || dest.batch_ != e.batch_)
        {
            dest.release();
            dest.ctx_ = e.ctx_;
            dest.batch_ = e.batch_;
        }
        dest.reshape_uninitialized(e.level(), e.size());
        dest.is_ntt_form() = e.is_ntt_form();
        dest.scale() = e.scale();
        dest.correction_factor() = e.correction_factor();
        return dest.data_;
    }

    void Evaluator::add_plain_device(const Ciphertext &e, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                     Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, plain, batch, plain_is_ntt, scale, dest);
        addsub_plain(e, PlainOperand(context_, e.level(), plain, plain_is_ntt, scale), 0, dest);
    }
    void Evaluator::sub_plain_device(const Ciphertext &e, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                     Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, plain, batch, plain_is_ntt, scale, dest);
        addsub_plain(e, PlainOperand(context_, e.level(), plain, plain_is_ntt, scale), 1, dest);
    }
    void Evaluator::multiply_plain_device(const Ciphertext &e, const uint64_t *plain, size_t batch, bool plain_is_ntt, double scale,
                                          Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, plain, batch, plain_is_ntt, scale, dest);
        multiply_plain(e, PlainOperand(context_, e.level(), plain, plain_is_ntt, scale), dest);
    }

    // dest <- e (+/-) plain (op 0 add, 1 sub); dest may be e
    void Evaluator::addsub_plain(const Ciphertext &e, const PlainOperand &plain, int op, Ciphertext &dest) const
    {
        check_addsub_plain_forms(e, plain.ntt, plain.level, plain.scale);
        const Level &lvl = *e.level();
        const size_t words = (size_t)lvl.K * context_.n();
        const unsigned n_log = (unsigned)context_.log_n(), K = lvl.K, batch = (unsigned)e.batch();
        const ModDesc *mods = context_.dev_mods();
        const uint64_t *a = e.plane(0);
        uint64_t *r = begin_result(e, dest);
        if (&dest != &e && e.size() > 1) // the other polynomials pass through
            ck(hipMemcpyAsync(r + e.plane_words(), e.plane(1), (e.size() - 1) * e.plane_words() * 8, hipMemcpyDeviceToDevice, stream_),
               "add/sub plain: copy c1..");
        switch (context_.scheme())
        {
        case Scheme::bfv:
            // multiply_add/sub_plain_with_scaling_variant (util/scalingvariant.cpp:70-175)
            ck(k_bfv_addsub_plain_batch(mods, bfv_plain_const(context_, lvl), plain.words, plain.stride, plain.coeff_count, a, r, op, n_log, K,
                                        batch, stream_),
               "bfv add/sub plain");
            break;
        case Scheme::ckks:
            ck(k_addsub_plain_batch(mods, a, plain.words, plain.stride, r, op, n_log, K, batch, stream_), "ckks add/sub plain");
            break;
        case Scheme::bgv:
            // plain * correction_factor mod t, lifted and transformed at the ciphertext's level (evaluator.cpp:1836-1847)
            lift_chunks(plain, lvl, e.correction_factor(), batch, nullptr, [&](size_t b0, unsigned items, const uint64_t *lifted, size_t stride) {
                ck(k_addsub_plain_batch(mods, a + b0 * words, lifted, stride, r + b0 * words, op, n_log, K, items, stream_), "bgv add/sub plain");
            });
            break;
        default:
            throw std::invalid_argument("unsupported scheme");
        }
        throw_if_transparent(dest);
    }

    // dest <- e * plain; dest may be e.  multiply_plain_ntt (evaluator.cpp:2157-2194), multiply_plain_normal (2021-2155) and the
    // mixed-form branches (2006-2017): whatever the forms, the product is taken in the NTT domain - a coefficient-form plaintext is
    // lifted and transformed at the ciphertext's level, a coefficient-form ciphertext is transformed and transformed back - except
    // for the monomial shortcut of multiply_plain_normal (2051-2095), which is not merely faster: with the "fast plain lift" (t
    // below every q_i) the reference multiplies by the RAW coefficient even when it lies in the upper half, i.e. by m instead of
    // m - t; the ciphertext words differ from the generic path (by t * ct * x^e), so the branch is reproduced, per item.  Costs one
    // read-back of 24 bytes per plaintext for a coefficient-form product.
    void Evaluator::multiply_plain(const Ciphertext &e, const PlainOperand &plain, Ciphertext &dest) const
    {
        const Level &lvl = *e.level();
        const bool ckks = context_.scheme() == Scheme::ckks, ct_ntt = e.is_ntt_form();
        if (plain.ntt && plain.level != &lvl)
            throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
        const size_t words = (size_t)lvl.K * context_.n(), size = e.size(), plane = e.plane_words(), batch = e.batch();
        const unsigned n_log = (unsigned)context_.log_n(), K = lvl.K;
        const ModDesc *mods = context_.dev_mods();
        const NttTables &tb = context_.ntt_tables();

        // the monomial branch, decided for every plaintext at once: one launch, one read-back
        std::unique_ptr<Scratch> stats;
        size_t monomials = 0;
        if (!ct_ntt && !plain.ntt && size)
        {
            const size_t count = plain.stride ? batch : 1;
            stats.reset(new Scratch(3 * count));
            ck(k_plain_stats_batch(plain.words, plain.stride, plain.coeff_count, stats->p, (unsigned)count, stream_), "plain stats");
            std::vector<uint64_t> st(3 * count);
            ck(hipMemcpyAsync(st.data(), stats->p, st.size() * 8, hipMemcpyDeviceToHost, stream_), "plain stats read");
            ck(hipStreamSynchronize(stream_), "plain stats sync");
            for (size_t b = 0; b < count; b++)
                monomials += st[3 * b] == 1;
            if (!plain.stride)
                monomials *= batch;
        }
        if (ckks && !plain.ntt && monomials < batch)
            throw std::invalid_argument("CKKS plain must be in NTT form");
        // as the reference: the scale is the plaintext's business wherever multiply_plain_ntt does the work, and in CKKS
        const bool scaled = ckks || ct_ntt || plain.ntt;
        const double new_scale = scaled ? e.scale() * plain.scale : e.scale();
        if (scaled && !scale_within_bounds(new_scale, lvl))
            throw std::invalid_argument("scale out of bounds");

        const uint64_t *src = e.data();
        // the monomial product permutes: in place it goes through a fresh slab
        uint64_t *fresh = (&dest == &e && monomials) ? DevicePool::global().alloc_words(e.word_count()) : nullptr;
        uint64_t *res = fresh ? fresh : begin_result(e, dest);
        try
        {
            if (monomials < batch && size)
            {
                if (!ct_ntt)
                {
                    NttBatch cb = plain_batch(res, words, K, (unsigned)(size * batch), 0);
                    if (res != src) // out of place: the first pass reads the operand itself (NttBatch::src, mode 0) - no copy
                    {
                        cb.src = src;
                        cb.src_outer_stride = words;
                        cb.src_ncomp = K;
                        cb.src_mode = 0;
                    }
                    // (a shared coefficient-form plaintext has always met lazy words here, the other shapes canonical ones: the
                    // product is the same canonical residue)
                    ck(ntt_forward(tb, cb, !plain.stride && !plain.ntt ? 1 : 0, stream_), "multiply_plain ntt");
                }
                const uint64_t *a = ct_ntt ? src : res;
                if (plain.ntt)
                    ck(k_dyadic_plain_batch(mods, a, plane, plain.words, plain.stride, res, plane, (unsigned)size, n_log, K, (unsigned)batch,
                                            stream_),
                       "multiply_plain");
                else // (the monomial items among them are overwritten below)
                    lift_chunks(plain, lvl, 1, batch, nullptr, [&](size_t b0, unsigned items, const uint64_t *lifted, size_t stride) {
                        ck(k_dyadic_plain_batch(mods, a + b0 * words, plane, lifted, stride, res + b0 * words, plane, (unsigned)size, n_log, K,
                                                items, stream_),
                           "multiply_plain");
                    });
                if (!ct_ntt)
                    ck(ntt_inverse(tb, plain_batch(res, words, K, (unsigned)(size * batch), 0), 0, stream_), "multiply_plain intt");
            }
            if (monomials)
                ck(k_negacyclic_mul_mono_batch(mods, stats->p, plain.stride ? 3 : 0, lvl.dev.plain_upper_half_threshold,
                                               fast_plain_lift(context_, lvl) ? nullptr : lvl.dev.upper_half_inc, src, plane, res, plane,
                                               (unsigned)size, n_log, K, (unsigned)batch, stream_),
                   "multiply_plain monomial");
        }
        catch (...)
        {
            DevicePool::global().free_words(fresh);
            throw;
        }
        if (fresh)
            dest.adopt(&lvl, size, fresh, e.word_count());
        dest.scale() = new_scale;
        throw_if_transparent(dest);
    }

    void Evaluator::transform_plain_to_ntt_device(const uint64_t *coefficients, size_t batch, const uint64_t *parms_id, uint64_t *out) const
    {
        StreamScope pool_scope(stream_);
        if (!coefficients || !out)
            throw std::invalid_argument("device pointer is null");
        if ((uintptr_t)coefficients % 16 || (uintptr_t)out % 16)
            throw std::invalid_argument("device pointers must be 16-byte aligned");
        if (!batch)
            throw std::invalid_argument("batch cannot be zero");
        const Level *lvl = context_.level_by_parms_id(parms_id);
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for the current context");
        if (context_.scheme() == Scheme::ckks)
            throw std::invalid_argument("CKKS plain must be in NTT form");
        const size_t n = context_.n();
        if (words_overlap(coefficients, batch * n * 8, out, batch * lvl->K * n * 8))
            throw std::invalid_argument("device_coefficients and device_words overlap");
        lift_chunks(PlainOperand(context_, lvl, coefficients, false, 1.0), *lvl, 1, batch, out, [](size_t, unsigned, const uint64_t *, size_t) {});
    }

    // ---- sums over the items of a device-resident batch (include/sealhip.h: Evaluator_SumItems / Evaluator_DotPlainDevice /
    // Evaluator_DotItems and their *Mapped forms).  A call is "rows output items and a walk": consecutive groups or an ItemMap
    ItemMap::ItemMap(const Context &context, uint64_t rows, const uint64_t *row_offsets, const uint64_t *first_items, const uint64_t *second_items,
                     uint64_t first_batch, uint64_t second_batch)
        : ctx_(&context), rows_((size_t)rows), first_batch_((size_t)first_batch), second_batch_((size_t)second_batch)
    {
        if (!row_offsets || !first_items)
            throw std::invalid_argument("row_offsets or first_items is null");
        if (!rows || rows >= (uint64_t(1) << 32))
            throw std::invalid_argument("1 <= rows < 2^32");
        if (row_offsets[0])
            throw std::invalid_argument("row_offsets[0] must be 0");
        for (uint64_t o = 0; o < rows; o++)
        {
            if (row_offsets[o + 1] <= row_offsets[o]) // add_many of nothing throws in the reference; the sum would be transparent
                throw std::invalid_argument("row_offsets must increase strictly: a row cannot be empty");
            longest_ = std::max<size_t>(longest_, (size_t)(row_offsets[o + 1] - row_offsets[o]));
        }
        const uint64_t terms = row_offsets[rows];
        if (terms >= (uint64_t(1) << 32))
            throw std::invalid_argument("terms < 2^32");
        if (!second_items && second_batch != first_batch)
            throw std::invalid_argument("one list of items: second_batch must equal first_batch");
        for (uint64_t t = 0; t < terms; t++)
            if (first_items[t] >= first_batch || (second_items && second_items[t] >= second_batch))
                throw std::invalid_argument("an item number is not below its batch");
        terms_ = (size_t)terms;
        // [rows + 1 offsets][terms][terms], each list padded to 16 bytes
        const auto pad4 = [](size_t n) { return (n + 3) & ~size_t(3); };
        const size_t off_at = 0, first_at = pad4(rows_ + 1), second_at = first_at + pad4(terms_);
        std::vector<uint32_t> host(second_items ? second_at + pad4(terms_) : second_at, 0);
        for (size_t o = 0; o <= rows_; o++)
            host[off_at + o] = (uint32_t)row_offsets[o];
        for (size_t t = 0; t < terms_; t++)
        {
            host[first_at + t] = (uint32_t)first_items[t];
            if (second_items)
                host[second_at + t] = (uint32_t)second_items[t];
        }
        block_ = DevicePool::global().alloc_words(host.size() / 2);
        try
        {
            ck(hipDeviceSynchronize(), "ItemMap upload"); // not a hot-path call: whatever used the block before is done
            copy_h2d(block_, host.data(), host.size() * 4);
        }
        catch (...)
        {
            DevicePool::global().free_words(block_);
            throw;
        }
        const uint32_t *base = reinterpret_cast<const uint32_t *>(block_);
        offsets_ = base + off_at;
        first_ = base + first_at;
        second_ = second_items ? base + second_at : first_;
    }
    ItemMap::~ItemMap()
    {
        DevicePool::global().free_words(block_); // tagged by the pool: work that still reads the lists is waited for by the next user
    }
    ItemWalk ItemMap::walk() const
    {
        return ItemWalk(longest_, (terms_ + rows_ - 1) / rows_, offsets_, first_, second_);
    }

    ItemWalk Evaluator::consecutive_walk(const Ciphertext &e, size_t group, size_t &rows) const
    {
        if (!group || e.batch() % group)
            throw std::invalid_argument("group must divide the ciphertext's batch");
        rows = e.batch() / group;
        return ItemWalk(group);
    }
    ItemWalk Evaluator::mapped_walk(const Ciphertext &e, const ItemMap &map, size_t &rows) const
    {
        if (map.context() != &context_)
            throw std::invalid_argument("item_map is not valid for the current context");
        if (e.batch() != map.first_batch())
            throw std::invalid_argument("the ciphertext's batch does not equal the map's first_batch");
        rows = map.rows();
        return map.walk();
    }
    void Evaluator::check_reduce_items(const Ciphertext &e, size_t rows, const Ciphertext &dest) const
    {
        if (&dest == &e)
            throw std::invalid_argument("destination must be different from encrypted");
        if (dest.batch() != rows)
            throw std::invalid_argument("destination's batch does not equal the number of output items");
    }
    // The one host path of the reductions, after their checks and with the operands settled: dest becomes `size` planes of `rows`
    // items at e's level with the given metadata, the cut is the library's rule for `threads` threads (one per output pair:
    // reduce_threads; a tile of rows per thread: dot_scalars_threads) and this walk, and launch(slices, scratch) starts the kernels
    template <class Launch>
    void Evaluator::reduce_items(const Ciphertext &e, size_t rows, const ItemWalk &walk, size_t size, size_t threads, bool ntt_form,
                                 double scale, uint64_t correction_factor, Ciphertext &dest, const char *what, Launch launch) const
    {
        const Level &lvl = *e.level();
        if (dest.ctx_ != e.ctx_)
        {
            dest.release();
            dest.ctx_ = e.ctx_;
        }
        dest.reshape_uninitialized(&lvl, size);
        dest.is_ntt_form() = ntt_form;
        dest.scale() = scale;
        dest.correction_factor() = correction_factor;
        const unsigned slices = batch_reduce_slices(threads, walk);
        std::unique_ptr<Scratch> scratch;
        if (slices > 1)
            scratch.reset(new Scratch(batch_reduce_scratch_words(slices, (unsigned)size, rows, (unsigned)context_.log_n(), lvl.K)));
        ck(launch(slices, scratch ? scratch->p : nullptr), what);
        throw_if_transparent(dest);
    }
    // one thread per output pair of grid_planes planes of `rows` items at e's level
    size_t Evaluator::reduce_threads(const Ciphertext &e, size_t rows, size_t grid_planes) const
    {
        return grid_planes * rows * e.level()->K * context_.n() / 2;
    }
    void Evaluator::sum_items(const Ciphertext &e, size_t rows, const ItemWalk &walk, Ciphertext &dest) const
    {
        check_reduce_items(e, rows, dest);
        e.settle(); // the operand's words are read by what follows
        // one thread per output pair, the planes in the grid
        reduce_items(e, rows, walk, e.size(), reduce_threads(e, rows, e.size()), e.is_ntt_form(), e.scale(), e.correction_factor(), dest, "sum (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_sum_items(context_.dev_mods(), e.data_, e.plane_words(), dest.data_, dest.plane_words(), (unsigned)e.size(),
                                            (unsigned)context_.log_n(), e.level()->K, rows, walk, slices, scratch, stream_);
                     });
    }
    void Evaluator::sum_items(const Ciphertext &e, size_t group, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        size_t rows;
        const ItemWalk walk = consecutive_walk(e, group, rows);
        sum_items(e, rows, walk, dest);
    }
    void Evaluator::sum_items_mapped(const Ciphertext &e, const ItemMap &map, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e, "encrypted");
        size_t rows;
        const ItemWalk walk = mapped_walk(e, map, rows);
        sum_items(e, rows, walk, dest);
    }
    // what the plaintext products over `rows` output items check once their operand is known: -> the result's scale
    double Evaluator::check_dot_plain(const Ciphertext &e, size_t rows, double scale, const Ciphertext &dest) const
    {
        check_reduce_items(e, rows, dest);
        // coefficient-form operands have no place in a reduction: the monomial branch of multiply_plain_normal is per item and data
        // dependent (include/sealhip.h)
        if (!e.is_ntt_form())
            throw std::invalid_argument("encrypted must be in NTT form");
        const bool ckks = context_.scheme() == Scheme::ckks;
        const double new_scale = ckks ? e.scale() * scale : e.scale(); // as multiply_plain_device
        if (ckks && !scale_within_bounds(new_scale, *e.level()))
            throw std::invalid_argument("scale out of bounds");
        return new_scale;
    }
    void Evaluator::dot_plain_items(const Ciphertext &e, const uint64_t *plain, size_t, size_t rows, const ItemWalk &walk, double scale,
                                    Ciphertext &dest) const
    {
        const double new_scale = check_dot_plain(e, rows, scale, dest);
        e.settle(); // the operand's words are read by what follows
        // one thread per output pair of one plane: the product loops over the planes
        reduce_items(e, rows, walk, e.size(), reduce_threads(e, rows, 1), e.is_ntt_form(), new_scale, e.correction_factor(), dest, "dot_plain (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_dot_plain_items(context_.dev_mods(), e.data_, e.plane_words(), plain, dest.data_, dest.plane_words(),
                                                  (unsigned)e.size(), (unsigned)context_.log_n(), e.level()->K, rows, walk, slices, scratch,
                                                  stream_);
                     });
    }
    void Evaluator::dot_plain_device(const Ciphertext &e, const uint64_t *plain, size_t batch, size_t group, double scale,
                                     Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, plain, batch, true, scale, dest);
        size_t rows;
        const ItemWalk walk = consecutive_walk(e, group, rows);
        dot_plain_items(e, plain, batch, rows, walk, scale, dest);
    }
    void Evaluator::dot_plain_mapped(const Ciphertext &e, const uint64_t *plain, size_t plain_count, const ItemMap &map, double scale,
                                     Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, plain, plain_count, true, scale, dest, false);
        if (plain_count != map.second_batch())
            throw std::invalid_argument("plain_count does not equal the map's second_batch");
        size_t rows;
        const ItemWalk walk = mapped_walk(e, map, rows);
        dot_plain_items(e, plain, plain_count, rows, walk, scale, dest);
    }

    // A dense rows x batch matrix of scalar plaintexts times the items of a batch (include/sealhip.h: Evaluator_DotScalarsDevice):
    // dot_plain_mapped over the dense map with [K] words per plaintext instead of [K][N] - its checks, metadata and settling - and
    // a kernel of its own, whose threads hold a tile of output rows (batch_reduce_kernels.h: k_dot_scalars)
    void Evaluator::dot_scalars_device(const Ciphertext &e, const uint64_t *scalars, size_t rows, size_t batch, double scale,
                                       Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        if (!rows || (rows >> 32) || (batch >> 32) || ((rows * batch) >> 32))
            throw std::invalid_argument("1 <= rows and rows * batch < 2^32");
        check_plain_device(e, scalars, batch, true, scale, dest, true, rows);
        const double new_scale = check_dot_plain(e, rows, scale, dest);
        e.settle(); // the operand's words are read by what follows
        const unsigned n_log = (unsigned)context_.log_n(), K = e.level()->K;
        reduce_items(e, rows, ItemWalk(batch), e.size(), dot_scalars_threads((unsigned)e.size(), rows, n_log, K), true, new_scale,
                     e.correction_factor(), dest, "dot_scalars", [&](unsigned slices, uint64_t *scratch) {
                         return k_dot_scalars(context_.dev_mods(), e.data_, e.plane_words(), scalars, dest.data_, dest.plane_words(),
                                              (unsigned)e.size(), n_log, K, rows, batch, slices, scratch, 0, stream_);
                     });
    }
    // A sparse matrix of scalar weights times the items of a batch (include/sealhip.h: Evaluator_DotScalarsMapped): dot_plain_mapped
    // with [K] words or one 32-bit integer per plaintext instead of [K][N] - its checks, metadata, settling and cut, the weights'
    // own extent in the overlap checks - and the scalar term of the same kernel (batch_reduce_kernels.h: k_dot_scalars_mapped)
    void Evaluator::dot_scalars_mapped(const Ciphertext &e, const void *weights, size_t weight_count, bool narrow, const ItemMap &map,
                                       double scale, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_plain_device(e, static_cast<const uint64_t *>(weights), weight_count, true, scale, dest, false, 1, narrow);
        if (weight_count != map.second_batch())
            throw std::invalid_argument("weight_count does not equal the map's second_batch");
        size_t rows;
        const ItemWalk walk = mapped_walk(e, map, rows);
        const double new_scale = check_dot_plain(e, rows, scale, dest);
        e.settle(); // the operand's words are read by what follows
        // one thread per output pair, the planes in the grid
        reduce_items(e, rows, walk, e.size(), reduce_threads(e, rows, e.size()), true, new_scale, e.correction_factor(), dest, "dot_scalars (mapped)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_dot_scalars_mapped(context_.dev_mods(), weights, narrow, e.data_, e.plane_words(), dest.data_, dest.plane_words(),
                                                     (unsigned)e.size(), (unsigned)context_.log_n(), e.level()->K, rows, walk, slices, scratch,
                                                     stream_);
                     });
    }
    // plaintext matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulPlainItems): dot_plain_mapped's checks, metadata and
    // settling over rows * cols output items that each add `inner` terms, and a kernel of its own, whose threads hold a tile of outputs
    void Evaluator::matmul_plain_items(const uint64_t *plain, const Ciphertext &e, size_t rows, size_t inner, size_t cols, bool second_transposed,
                                       bool result_transposed, double scale, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_matmul_shape(rows, inner, cols);
        check_plain_device(e, plain, rows * inner, true, scale, dest, false);
        if (e.batch() != inner * cols)
            throw std::invalid_argument("the ciphertext's batch does not equal inner * cols");
        const double new_scale = check_dot_plain(e, rows * cols, scale, dest);
        const unsigned n_log = (unsigned)context_.log_n(), K = e.level()->K;
        const size_t threads = matmul_plain_items_threads((unsigned)e.size(), rows, cols, n_log, K);
        if (!threads)
            throw std::invalid_argument("the result is too large for one launch");
        e.settle(); // the operand's words are read by what follows
        reduce_items(e, rows * cols, ItemWalk(inner), e.size(), threads, true, new_scale, e.correction_factor(), dest, "matmul_plain (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_matmul_plain_items(context_.dev_mods(), plain, e.data_, e.plane_words(), dest.data_, dest.plane_words(),
                                                     (unsigned)e.size(), n_log, K, rows, inner, cols, second_transposed, result_transposed,
                                                     slices, scratch, 0, stream_);
                     });
    }
    // scalar weight matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulScalarsItems): matmul_plain_items with [K] words or
    // one 32-bit integer per plaintext instead of [K][N] - its checks, metadata and settling - and dot_scalars_device's kind of kernel
    void Evaluator::matmul_scalars_items(const void *weights, bool narrow, const Ciphertext &e, size_t rows, size_t inner, size_t cols,
                                         bool second_transposed, bool result_transposed, double scale, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_matmul_shape(rows, inner, cols);
        check_plain_device(e, static_cast<const uint64_t *>(weights), inner, true, scale, dest, false, rows, narrow);
        if (e.batch() != inner * cols)
            throw std::invalid_argument("the ciphertext's batch does not equal inner * cols");
        const double new_scale = check_dot_plain(e, rows * cols, scale, dest);
        const unsigned n_log = (unsigned)context_.log_n(), K = e.level()->K;
        const size_t threads = matmul_scalars_threads((unsigned)e.size(), rows, cols, n_log, K, narrow);
        if (!threads)
            throw std::invalid_argument("the result is too large for one launch");
        e.settle(); // the operand's words are read by what follows
        reduce_items(e, rows * cols, ItemWalk(inner), e.size(), threads, true, new_scale, e.correction_factor(), dest, "matmul_scalars (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_matmul_scalars(context_.dev_mods(), weights, narrow, e.data_, e.plane_words(), dest.data_, dest.plane_words(),
                                                 (unsigned)e.size(), n_log, K, rows, inner, cols, second_transposed, result_transposed, slices,
                                                 scratch, 0, stream_);
                     });
    }
    // 2-D convolution of scalar weights over a grid of items (include/sealhip.h: Evaluator_Conv2dScalarsItems): matmul_scalars_items
    // with rows = OC, inner = C * kh * kw and cols = OH * OW - its checks, metadata, settling and cut - and a kernel that finds the
    // operand of a term in the image instead of in a gathered batch
    void Evaluator::conv2d_scalars_items(const void *weights, bool narrow, const Ciphertext &e, const Conv2dShape &shape, bool in_last,
                                         bool out_last, double scale, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        size_t oh, ow;
        if (const char *wrong = conv2d_shape_error(shape, oh, ow))
            throw std::invalid_argument(wrong);
        const size_t rows = shape.out_channels, inner = shape.in_channels * shape.kernel_h * shape.kernel_w, cols = oh * ow;
        check_plain_device(e, static_cast<const uint64_t *>(weights), inner, true, scale, dest, false, rows, narrow);
        if (e.batch() != shape.in_channels * shape.height * shape.width)
            throw std::invalid_argument("the ciphertext's batch does not equal in_channels * height * width");
        const double new_scale = check_dot_plain(e, rows * cols, scale, dest);
        const unsigned n_log = (unsigned)context_.log_n(), K = e.level()->K;
        const size_t threads = conv2d_scalars_threads((unsigned)e.size(), shape, n_log, K, narrow);
        if (!threads)
            throw std::invalid_argument("the result is too large for one launch");
        e.settle(); // the operand's words are read by what follows
        reduce_items(e, rows * cols, ItemWalk(inner), e.size(), threads, true, new_scale, e.correction_factor(), dest, "conv2d_scalars (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_conv2d_scalars(context_.dev_mods(), weights, narrow, e.data_, e.plane_words(), dest.data_, dest.plane_words(),
                                                 (unsigned)e.size(), n_log, K, shape, in_last, out_last, slices, scratch, 0, 0, stream_);
                     });
    }
    // BFV / BGV scalars (include/sealhip.h: Evaluator_LiftScalars): the centred lift of transform_to_ntt_inplace(Plaintext) for the
    // constant polynomial m - m mod q_k, plus (Q - t) mod q_k from the upper-half threshold on, in both lift branches of the reference
    // (evaluator.cpp:2243-2282) - and the forward transform of a constant is that constant at every position
    void Evaluator::lift_scalars(size_t count, const uint64_t *values, const uint64_t *parms_id, uint64_t *words) const
    {
        StreamScope pool_scope(stream_);
        if (!values || !words)
            throw std::invalid_argument(values ? "device_words cannot be null" : "values cannot be null");
        if ((uintptr_t)words % 16)
            throw std::invalid_argument("device_words must be 16-byte aligned");
        if (!count)
            throw std::invalid_argument("count cannot be zero");
        const Level *lvl = context_.level_by_parms_id(parms_id);
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for the current context");
        if (context_.scheme() == Scheme::ckks)
            throw std::invalid_argument("CKKS plain must be in NTT form");
        const uint64_t t = context_.plain_modulus(), threshold = (t + 1) >> 1;
        std::vector<uint64_t> host(count * lvl->K);
        for (size_t i = 0; i < count; i++)
        {
            if (values[i] >= t)
                throw std::invalid_argument("a value is not below the plain modulus (values[" + std::to_string(i) + "])");
            for (unsigned k = 0; k < lvl->K; k++)
            {
                const uint64_t q = context_.coeff_modulus()[k], inc = (q - t % q) % q, v = values[i] % q;
                host[i * lvl->K + k] = values[i] >= threshold ? (v + inc) % q : v;
            }
        }
        ck(hipDeviceSynchronize(), "scalars upload"); // not a hot-path call: whatever read or wrote the buffer before is done
        copy_h2d(words, host.data(), host.size() * 8);
    }

    // sum over the terms of an output item of the 2 x 2 tensor products (include/sealhip.h: Evaluator_DotItems): the checks and
    // metadata of multiply (ckks_multiply / bgv_multiply at 2 x 2) and of sum_items, one kernel and no stored product.  The batches
    // of the operands are the walk's business and checked by the callers
    void Evaluator::check_dot_items(const Ciphertext &e1, const Ciphertext &e2, size_t rows, const Ciphertext &dest, double &new_scale,
                                    uint64_t &cf) const
    {
        if (e1.level() != e2.level())
            throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        if (!(e1.is_ntt_form() && e2.is_ntt_form()))
            throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
        if (e1.size() != 2 || e2.size() != 2)
            throw std::invalid_argument("encrypted1 and encrypted2 must have size 2");
        check_reduce_items(e1, rows, dest);
        if (&dest == &e2)
            throw std::invalid_argument("destination must be different from encrypted");
        const bool ckks = context_.scheme() == Scheme::ckks;
        new_scale = ckks ? e1.scale() * e2.scale() : e1.scale();
        if (ckks && !scale_within_bounds(new_scale, *e1.level()))
            throw std::invalid_argument("scale out of bounds");
        cf = ckks ? 1 : host::mulmod(e1.correction_factor(), e2.correction_factor(), context_.plain_modulus());
    }
    void Evaluator::dot_items(const Ciphertext &e1, const Ciphertext &e2, size_t rows, const ItemWalk &walk, Ciphertext &dest) const
    {
        double new_scale;
        uint64_t cf;
        check_dot_items(e1, e2, rows, dest, new_scale, cf);
        const Level &lvl = *e1.level();
        // operands first: whatever is pending on them (a key-switch tail, a product of their own) is settled before their words are read
        const uint64_t *xw = e1.data(), *yw = &e1 == &e2 ? xw : e2.data();
        reduce_items(e1, rows, walk, 3, reduce_threads(e1, rows, 1), true, new_scale, cf, dest, "dot (items)", [&](unsigned slices, uint64_t *scratch) {
            return k_dot_items(context_.dev_mods(), xw, e1.plane_words(), yw, e2.plane_words(), dest.data_, dest.plane_words(),
                               (unsigned)context_.log_n(), lvl.K, rows, walk, slices, scratch, stream_);
        });
    }
    // what both forms check before they know their walk
    static void check_dot_items_scheme(Scheme scheme)
    {
        // BFV's product rounds per item (BEHZ): the sum of the rounded products is not the rounded sum
        if (scheme != Scheme::ckks && scheme != Scheme::bgv)
            throw std::invalid_argument("unsupported scheme");
    }
    void Evaluator::dot_items(const Ciphertext &e1, const Ciphertext &e2, size_t group, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e1, "encrypted1");
        check_valid(e2, "encrypted2");
        check_dot_items_scheme(context_.scheme());
        if (e1.batch() != e2.batch())
            throw std::invalid_argument("batch mismatch");
        size_t rows;
        const ItemWalk walk = consecutive_walk(e1, group, rows);
        dot_items(e1, e2, rows, walk, dest);
    }
    void Evaluator::dot_items_mapped(const Ciphertext &e1, const Ciphertext &e2, const ItemMap &map, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e1, "encrypted1");
        check_valid(e2, "encrypted2");
        check_dot_items_scheme(context_.scheme());
        if (e2.batch() != map.second_batch())
            throw std::invalid_argument("encrypted2's batch does not equal the map's second_batch");
        size_t rows;
        const ItemWalk walk = mapped_walk(e1, map, rows);
        dot_items(e1, e2, rows, walk, dest);
    }

    // ciphertext matrix x ciphertext matrix (include/sealhip.h: Evaluator_MatMulItems): dot_items' checks, metadata and settling over
    // rows * cols output items that each add `inner` terms, and a kernel of its own, whose threads hold a tile of outputs
    void Evaluator::matmul_items(const Ciphertext &e1, const Ciphertext &e2, size_t rows, size_t inner, size_t cols, bool second_transposed,
                                 Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        check_valid(e1, "encrypted1");
        check_valid(e2, "encrypted2");
        check_dot_items_scheme(context_.scheme());
        check_matmul_shape(rows, inner, cols);
        if (e1.batch() != rows * inner || e2.batch() != inner * cols)
            throw std::invalid_argument("batch mismatch");
        double new_scale;
        uint64_t cf;
        check_dot_items(e1, e2, rows * cols, dest, new_scale, cf);
        const unsigned n_log = (unsigned)context_.log_n(), K = e1.level()->K;
        const size_t threads = matmul_items_threads(rows, cols, n_log, K);
        if (!threads)
            throw std::invalid_argument("the result is too large for one launch");
        // operands first: whatever is pending on them (a key-switch tail, a product of their own) is settled before their words are read
        const uint64_t *xw = e1.data(), *yw = &e1 == &e2 ? xw : e2.data();
        reduce_items(e1, rows * cols, ItemWalk(inner), 3, threads, true, new_scale, cf, dest, "matmul (items)",
                     [&](unsigned slices, uint64_t *scratch) {
                         return k_matmul_items(context_.dev_mods(), xw, e1.plane_words(), yw, e2.plane_words(), dest.data_, dest.plane_words(),
                                               n_log, K, rows, inner, cols, second_transposed, slices, scratch, 0, stream_);
                     });
    }

    void Evaluator::add_many(const std::vector<const Ciphertext *> &encrypteds, Ciphertext &destination) const
    {
        StreamScope pool_scope(stream_);
        if (encrypteds.empty())
            throw std::invalid_argument("encrypteds cannot be empty");
        for (const Ciphertext *c : encrypteds)
            if (!c || c == &destination)
                throw std::invalid_argument("encrypteds must be different from destination");
        destination = *encrypteds[0];
        for (size_t i = 1; i < encrypteds.size(); i++)
            add_inplace(destination, *encrypteds[i]);
    }

    void Evaluator::multiply_many(const std::vector<const Ciphertext *> &encrypteds, const KSwitchKeys &relin_keys, Ciphertext &destination) const
    {
        StreamScope pool_scope(stream_);
        // the product tree of evaluator.cpp:1649-1723, every product relinearized
        if (encrypteds.empty())
            throw std::invalid_argument("encrypteds vector must not be empty");
        for (const Ciphertext *c : encrypteds)
            if (!c || c == &destination)
                throw std::invalid_argument("encrypteds must be different from destination");
        check_context(*encrypteds[0], "encrypteds");
        if (context_.scheme() != Scheme::bfv && context_.scheme() != Scheme::bgv)
            throw std::logic_error("unsupported scheme");
        if (encrypteds.size() == 1)
        {
            destination = *encrypteds[0];
            return;
        }
        std::vector<std::unique_ptr<Ciphertext>> owned;
        std::vector<const Ciphertext *> prod;
        for (size_t i = 0; i + 1 < encrypteds.size(); i += 2)
        {
            std::unique_ptr<Ciphertext> temp(new Ciphertext(context_, encrypteds[i]->batch()));
            if (encrypteds[i]->data() == encrypteds[i + 1]->data())
            {
                *temp = *encrypteds[i];
                square_inplace(*temp);
            }
            else
                multiply(*encrypteds[i], *encrypteds[i + 1], *temp);
            relinearize_inplace(*temp, relin_keys);
            prod.push_back(temp.get());
            owned.push_back(std::move(temp));
        }
        if (encrypteds.size() & 1)
            prod.push_back(encrypteds.back());
        for (size_t i = 0; i + 1 < prod.size(); i += 2)
        {
            std::unique_ptr<Ciphertext> temp(new Ciphertext(context_, prod[i]->batch()));
            multiply(*prod[i], *prod[i + 1], *temp);
            relinearize_inplace(*temp, relin_keys);
            prod.push_back(temp.get());
            owned.push_back(std::move(temp));
        }
        destination = *prod.back();
    }

    void Evaluator::exponentiate_inplace(Ciphertext &e, uint64_t exponent, const KSwitchKeys &relin_keys) const
    {
        StreamScope pool_scope(stream_);
        check_context(e);
        if (relin_keys.context() != &context_)
            throw std::invalid_argument("relin_keys is not valid for encryption parameters");
        if (exponent == 0)
            throw std::invalid_argument("exponent cannot be 0");
        if (exponent == 1)
            return;
        // multiply_many over `exponent` copies (evaluator.cpp:1725-1757); the copies share one buffer here, so the
        // first tree level squares it, exactly as the reference does for identical operands
        Ciphertext base(e);
        std::vector<const Ciphertext *> v((size_t)exponent, &base);
        multiply_many(v, relin_keys, e);
    }

    // ---- multiply (evaluator.cpp:352-708)
    void Evaluator::check_product_operands(const Ciphertext &e1, const Ciphertext &e2) const
    {
        check_valid(e1, "encrypted1");
        check_valid(e2, "encrypted2");
        if (e1.level() != e2.level())
            throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        if (e1.batch() != e2.batch())
            throw std::invalid_argument("batch mismatch");
    }
    size_t Evaluator::product_size(size_t s1, size_t s2) const
    {
        if (s1 < 2 || s2 < 2)
            throw std::invalid_argument("encrypted size must be at least 2");
        if (s1 + s2 - 1 > 16)
            throw std::logic_error("invalid parameters");
        return s1 + s2 - 1;
    }
    void Evaluator::multiply_inplace(Ciphertext &e1, const Ciphertext &e2) const
    {
        StreamScope pool_scope(stream_);
        check_product_operands(e1, e2);
        switch (context_.scheme())
        {
        case Scheme::bfv:
            bfv_multiply_to(e1, e2, e1);
            break;
        case Scheme::ckks:
            ckks_multiply(e1, e2);
            break;
        case Scheme::bgv:
            bgv_multiply(e1, e2);
            break;
        default:
            throw std::invalid_argument("unsupported scheme");
        }
        throw_if_transparent(e1);
    }
    void Evaluator::multiply(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &dest) const
    {
        StreamScope pool_scope(stream_);
        // evaluator.h:239-247: destination = encrypted1; multiply_inplace(destination, encrypted2).
        // Device-resident fast path: the common size-2 x size-2 CKKS product writes the three result
        // polynomials straight into `dest` instead of copying encrypted1 first.
        if (&dest == &e1)
            return multiply_inplace(dest, e2);
        if (&dest == &e2)
            return multiply_inplace(dest, e1);
        if (context_.scheme() == Scheme::ckks && e1.size() == 2 && e2.size() == 2 && &dest.context() == &context_ &&
            dest.batch() == e1.batch())
        {
            check_product_operands(e1, e2);
            if (!(e1.is_ntt_form() && e2.is_ntt_form()))
                throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
            const Level &lvl = *e1.level();
            PlaneGeom g{ (unsigned)context_.log_n(), lvl.K, (unsigned)e1.batch() };
            // operands first: whatever is pending on them (a key-switch tail, a product of their own) is settled before their words are
            // read - now or by the deferred product
            const uint64_t *xw = e1.data(), *yw = e2.data();
            dest.reshape_uninitialized(&lvl, 3);
            // Round 6: batches whose key switch runs un-split at a two-pass size - the product is not formed now (LazyProduct): a
            // relinearize_inplace that follows forms it inside its own kernels, anything else that needs the words forms it first
            const bool defer = may_defer_product(lvl, e1.batch());
            if (defer)
                defer_product(dest, &e1, &e2, nullptr);
            else
                ck(k_ckks_multiply_2x2(context_.dev_mods(), context_.ntt_tables().fpd, nullptr, xw, yw, dest.data(), g, stream_), "ckks_multiply");
            dest.is_ntt_form() = true;
            dest.correction_factor() = 1;
            dest.scale() = e1.scale() * e2.scale();
            if (!scale_within_bounds(dest.scale(), lvl))
                throw std::invalid_argument("scale out of bounds");
            throw_if_transparent(dest);
            return;
        }
        if (context_.scheme() == Scheme::bfv && &dest.context() == &context_ && dest.batch() == e1.batch())
        {
            // BFV: the same checks as multiply_inplace, then the product straight into `dest` (no copy of encrypted1: 6.8 GB per
            // step at BASELINE configs[3])
            check_product_operands(e1, e2);
            bfv_multiply_to(e1, e2, dest);
            dest.is_ntt_form() = false;
            dest.scale() = e1.scale();
            dest.correction_factor() = e1.correction_factor();
            throw_if_transparent(dest);
            return;
        }
        dest = e1;
        if (&e1 == &e2)
            multiply_inplace(dest, dest);
        else
            multiply_inplace(dest, e2);
    }

    void Evaluator::square_inplace(Ciphertext &e) const
    {
        StreamScope pool_scope(stream_);
        // ckks_square / bfv_square compute (c0^2, 2 c0 c1, c1^2) = the product of e with itself
        // (evaluator.cpp:878-1142); canonical results coincide with multiply(e, e).
        check_valid(e, "encrypted");
        multiply_inplace(e, e);
    }

    // e1 <- the tensor product of the NTT-form operands e1 and e2, `size` polynomials (evaluator.cpp:626-707, 760-841).  The common
    // (c0, c1) x (d0, d1) is formed in place when e1's slab has room (every thread reads its four words before it writes its three);
    // everything else goes straight into a new slab that e1 adopts - no copy of the old polynomials, no zeroing of the new ones.
    void Evaluator::tensor_ntt(Ciphertext &e1, const Ciphertext &e2, size_t size) const
    {
        expect_scope();
        const Level &lvl = *e1.level();
        const PlaneGeom g{ (unsigned)context_.log_n(), lvl.K, (unsigned)e1.batch() };
        const size_t words = size * g.words();
        const uint64_t *x = e1.data(), *y = (&e1 == &e2) ? x : e2.data(); // (completes a pending key-switch tail)
        if (size == 3 && e1.capacity_words() >= words)
        {
            e1.reshape_uninitialized(&lvl, 3); // enough room: the words stay where they are
            ck(k_ckks_multiply_2x2(context_.dev_mods(), context_.ntt_tables().fpd, nullptr, x, y, e1.data(), g, stream_), "multiply 2x2");
            return;
        }
        uint64_t *out = DevicePool::global().alloc_words(words, stream_);
        if (size == 3)
            ck(k_ckks_multiply_2x2(context_.dev_mods(), context_.ntt_tables().fpd, nullptr, x, y, out, g, stream_), "multiply 2x2");
        else
            ck(k_multiply_general(context_.dev_mods(), nullptr, x, (unsigned)e1.size(), y, (unsigned)e2.size(), out, g, stream_),
               context_.scheme() == Scheme::ckks ? "ckks_multiply general" : "bgv_multiply general");
        e1.adopt(&lvl, size, out, words);
    }

    void Evaluator::ckks_multiply(Ciphertext &e1, const Ciphertext &e2) const
    {
        expect_scope();
        if (!(e1.is_ntt_form() && e2.is_ntt_form()))
            throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
        const Level &lvl = *e1.level();
        const size_t size = product_size(e1.size(), e2.size());
        const double new_scale = e1.scale() * e2.scale();
        if (size == 3 && may_defer_product(lvl, e1.batch()))
        {
            // Round 6 (LazyProduct, in place): e1's slab - its two polynomials as they are now, whatever was pending on them completed -
            // goes to the record, e1 gets a fresh slab of three whose words are pending.  Nothing is copied and nothing is computed here.
            const bool self = (&e1 == &e2);
            (void)e1.data();
            if (!self)
                (void)e2.data();
            const size_t words = 3 * e1.plane_words();
            uint64_t *fresh = DevicePool::global().alloc_words(words, stream_);
            uint64_t *old = e1.exchange_slab(&lvl, 3, fresh, words);
            defer_product(e1, nullptr, self ? nullptr : &e2, old);
        }
        else
            tensor_ntt(e1, e2, size);
        e1.scale() = new_scale;
        if (!scale_within_bounds(e1.scale(), lvl))
            throw std::invalid_argument("scale out of bounds");
    }

    // bgv_multiply / bgv_square (evaluator.cpp:710-841, 1079-1142): the tensor product of ckks_multiply on
    // NTT-form operands; the scale is untouched and the correction factors multiply modulo t.
    void Evaluator::bgv_multiply(Ciphertext &e1, const Ciphertext &e2) const
    {
        if (!(e1.is_ntt_form() && e2.is_ntt_form()))
            throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
        const size_t size = product_size(e1.size(), e2.size());
        const uint64_t cf = host::mulmod(e1.correction_factor(), e2.correction_factor(), context_.plain_modulus());
        tensor_ntt(e1, e2, size);
        e1.correction_factor() = cf;
    }

    // the product of e1 and e2 into dest (dest may be e1): BEHZ reads its operands through the first transform pass and builds the
    // result in a new slab, so an out-of-place product needs no copy of e1 (evaluator.h:239-247 copies it first)
    void Evaluator::bfv_multiply_to(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &dst) const
    {
        expect_scope();
        if (e1.is_ntt_form() || e2.is_ntt_form())
            throw std::invalid_argument("encrypted1 or encrypted2 cannot be in NTT form");
        const Level &lvl = *e1.level();
        const LevelDev &lv = lvl.dev;
        const unsigned K = lvl.K, nBsk = lv.nBsk;
        const size_t N = context_.n(), B = e1.batch();
        const unsigned n_log = (unsigned)context_.log_n();
        const size_t s1 = e1.size(), s2 = e2.size(), dest = product_size(s1, s2);
        const bool self = (&e1 == &e2);
        const NttTables &tb = context_.ntt_tables();
        const ModDesc *mods = context_.dev_mods();

        // steps (1)-(3): lift each input to q U Bsk and transform (evaluator.cpp:456-489)
        auto lift = [&](const Ciphertext &x, Scratch &xq, Scratch &xb) {
            size_t items = x.size() * B;
            // out of place: the first pass reads the ciphertext itself (NttBatch::src, mode 0) - no copy of the input
            NttBatch qb = plain_batch(xq.p, (size_t)K * N, K, (unsigned)items, 0);
            qb.src = x.data();
            qb.src_outer_stride = (size_t)K * N;
            qb.src_ncomp = K;
            qb.src_mode = 0;
            ck(ntt_forward(tb, qb, 0, stream_), "bfv ntt q");
            ck(k_behz_lift(mods, lv, x.data(), xb.p, n_log, items, stream_), "behz lift");
            NttBatch bb = plain_batch(xb.p, (size_t)nBsk * N, nBsk, (unsigned)items, 0);
            bb.comp_prime = lv.bsk_prime;
            bb.cls_hint = 0; // the auxiliary base is 61-bit primes: integer back end, single-class kernels (ntt_kernels.h)
            ck(ntt_forward(tb, bb, 0, stream_), "bfv ntt Bsk");
        };
        Scratch x_q(s1 * B * K * N), x_b(s1 * B * nBsk * N);
        lift(e1, x_q, x_b);
        std::unique_ptr<Scratch> y_q, y_b;
        if (!self)
        {
            y_q.reset(new Scratch(s2 * B * K * N));
            y_b.reset(new Scratch(s2 * B * nBsk * N));
            lift(e2, *y_q, *y_b);
        }
        const uint64_t *yq = self ? x_q.p : y_q->p;
        const uint64_t *yb = self ? x_b.p : y_b->p;

        // step (4): dyadic ciphertext product in both bases (evaluator.cpp:497-541)
        Scratch d_q(dest * B * K * N), d_b(dest * B * nBsk * N);
        PlaneGeom gq{ n_log, K, (unsigned)B }, gb{ n_log, nBsk, (unsigned)B };
        // Two-pass sizes, 2 x 2: steps (4) and (5) are ONE pair of passes per base - the inverse transform's first pass forms the
        // product from the four operand polynomials as it loads them (NttBatch::prod_x), so the product is never stored in NTT form
        // and read back: 7 plane crossings instead of 13 (profiles/r04_bfv_product_source.txt).  ntt2_supports chooses that or the stored product.
        const bool product_source = s1 == 2 && s2 == 2 && ntt2_supports(context_.log_n());
        if (product_source)
        {
            NttBatch iq = plain_batch(d_q.p, (size_t)K * N, K, (unsigned)(3 * B), 0);
            iq.prod_x = x_q.p;
            iq.prod_y = yq;
            iq.prod_batch = (unsigned)B;
            iq.src_outer_stride = (size_t)K * N;
            ck(ntt_inverse(tb, iq, 0, stream_), "bfv tensor + intt q");
            NttBatch ibp = plain_batch(d_b.p, (size_t)nBsk * N, nBsk, (unsigned)(3 * B), 0);
            ibp.comp_prime = lv.bsk_prime;
            ibp.cls_hint = 0;
            ibp.prod_x = x_b.p;
            ibp.prod_y = yb;
            ibp.prod_batch = (unsigned)B;
            ibp.src_outer_stride = (size_t)nBsk * N;
            ck(ntt_inverse(tb, ibp, 0, stream_), "bfv tensor + intt Bsk");
        }
        else if (s1 == 2 && s2 == 2)
        {
            // the common product: four loads, three reductions per coefficient (the general kernel: eight and four); the transforms
            // around it leave canonical words, primes below 2^50 take the double-precision products, the 61-bit auxiliary base does not
            ck(k_ckks_multiply_2x2(mods, tb.fpd, nullptr, x_q.p, yq, d_q.p, gq, stream_), "bfv tensor q");
            ck(k_ckks_multiply_2x2(mods, tb.fpd, lv.bsk_prime, x_b.p, yb, d_b.p, gb, stream_), "bfv tensor Bsk");
        }
        else
        {
            ck(k_multiply_general(mods, nullptr, x_q.p, (unsigned)s1, yq, (unsigned)s2, d_q.p, gq, stream_), "bfv tensor q");
            ck(k_multiply_general(mods, lv.bsk_prime, x_b.p, (unsigned)s1, yb, (unsigned)s2, d_b.p, gb, stream_), "bfv tensor Bsk");
        }

        // step (5): back to coefficient form
        if (!product_source)
        {
            ck(ntt_inverse(tb, plain_batch(d_q.p, (size_t)K * N, K, (unsigned)(dest * B), 0), 0, stream_), "bfv intt q");
            NttBatch ib = plain_batch(d_b.p, (size_t)nBsk * N, nBsk, (unsigned)(dest * B), 0);
            ib.comp_prime = lv.bsk_prime;
            ib.cls_hint = 0;
            ck(ntt_inverse(tb, ib, 0, stream_), "bfv intt Bsk");
        }

        // steps (6)-(8)
        size_t words = dest * B * K * N;
        uint64_t *out = DevicePool::global().alloc_words(words);
        ck(k_behz_floor_sk(mods, lv, d_q.p, d_b.p, out, n_log, dest * B, stream_), "behz floor_sk");
        dst.adopt(&lvl, dest, out, words);
    }

} // namespace sealhip
