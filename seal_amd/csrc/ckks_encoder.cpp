// See ckks_encoder.h.  Reference: native/src/seal/ckks.h, ckks.cpp, util/croots.cpp, util/rns.cpp (RNSBase).
#include "ckks_encoder.h"
#include "hostmath.h"
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <string>

namespace sealhip
{
    namespace
    {
        void ck(hipError_t e, const char *what)
        {
            if (e != hipSuccess)
                throw std::runtime_error(std::string("HIP failure in ") + what + ": " + hipGetErrorString(e));
        }
        // util::ComplexRoots (croots.cpp:12-70)
        struct ComplexRoots
        {
            size_t degree;
            std::vector<std::complex<double>> roots;
            explicit ComplexRoots(size_t degree_of_roots) : degree(degree_of_roots), roots(degree_of_roots / 8 + 1)
            {
                constexpr double PI_ = 3.1415926535897932384626433832795028842;
                // std::polar(1.0, theta) = (cos theta, sin theta).  The reference is compiled with GCC, which fuses the two calls
                // into one sincos(); glibc's sincos and its separate sin / cos are not bit-identical for every argument, and
                // clang (hipcc's host compiler) does not fuse - so the fused call is made explicitly here.
                for (size_t i = 0; i <= degree / 8; i++)
                {
                    const double theta = 2 * PI_ * static_cast<double>(i) / static_cast<double>(degree);
                    double sn, cs;
                    ::sincos(theta, &sn, &cs);
                    roots[i] = std::complex<double>(1.0 * cs, 1.0 * sn);
                }
            }
            std::complex<double> get_root(size_t index) const
            {
                index &= degree - 1;
                auto mirror = [](std::complex<double> a) { return std::complex<double>{ a.imag(), a.real() }; };
                if (index <= degree / 8)
                    return roots[index];
                if (index <= degree / 4)
                    return mirror(roots[degree / 4 - index]);
                if (index <= degree / 2)
                    return -std::conj(get_root(degree / 2 - index));
                if (index <= 3 * degree / 4)
                    return -get_root(index - degree / 2);
                return std::conj(get_root(degree - index));
            }
        };
        // encode_internal rejects a vector whose largest |coefficient| c has safe_ceil_log2_int(max(c, 1.0)) + 1 >=
        // total_coeff_modulus_bit_count (ckks.h:525-548).  The largest c that passes, found once per level with the same libm
        // log2 the reference calls (monotonic), lets the kernels decide per coefficient with one comparison: fail iff
        // !(|c| <= limit), which also catches NaN and infinity.
        double coeff_limit(int total_bits)
        {
            if (total_bits < 2)
                return -1.0;
            auto passes = [total_bits](double x) { return static_cast<int>(std::ceil(std::log2(x))) + 1 < total_bits; };
            uint64_t lo, hi;
            const double dlo = std::ldexp(1.0, total_bits - 2), dhi = std::ldexp(1.0, total_bits - 1);
            std::memcpy(&lo, &dlo, 8);
            std::memcpy(&hi, &dhi, 8);
            while (hi - lo > 1) // passes(lo), !passes(hi); positive doubles order like their bit patterns
            {
                const uint64_t mid = lo + (hi - lo) / 2;
                double x;
                std::memcpy(&x, &mid, 8);
                (passes(x) ? lo : hi) = mid;
            }
            double limit;
            std::memcpy(&limit, &lo, 8);
            return limit;
        }
        uint32_t reverse_bits(uint64_t v, int bits)
        {
            uint64_t r = 0;
            for (int b = 0; b < bits; b++)
                r |= ((v >> b) & 1) << (bits - 1 - b);
            return (uint32_t)r;
        }
    } // namespace

    CKKSEncoder::CKKSEncoder(const Context &context) : context_(context)
    {
        if (context.scheme() != Scheme::ckks)
            throw std::invalid_argument("unsupported scheme");
        const size_t n = context.n();
        const int logn = context.log_n();
        if (logn < 1 || logn > (int)(kFftLdsLog + kFftMaxColumnLog))
            throw std::invalid_argument("poly_modulus_degree is not supported by the CKKS encoder");
        slots_ = n >> 1;
        std::vector<uint32_t> map(n);
        const uint64_t m = (uint64_t)n << 1;
        uint64_t pos = 1;
        for (size_t i = 0; i < slots_; i++)
        {
            map[i] = reverse_bits((pos - 1) >> 1, logn);
            map[slots_ | i] = reverse_bits((m - pos - 1) >> 1, logn);
            pos = (pos * 3) & (m - 1);
        }
        std::vector<std::complex<double>> rp(n), irp(n);
        if (m >= 8)
        {
            ComplexRoots cr((size_t)m);
            for (size_t i = 1; i < n; i++)
            {
                rp[i] = cr.get_root(reverse_bits(i, logn));
                irp[i] = std::conj(cr.get_root((size_t)reverse_bits(i - 1, logn) + 1));
            }
        }
        else if (m == 4)
        {
            rp[1] = { 0, 1 };
            irp[1] = { 0, -1 };
        }
        // the kernels walk coefficient positions: position -> slot (< N/2) or conjugate slot (>= N/2)
        std::vector<uint32_t> inv(n);
        for (size_t i = 0; i < n; i++)
            inv[map[i]] = (uint32_t)i;
        ck(hipMalloc(reinterpret_cast<void **>(&inv_map_), n * 4), "hipMalloc ckks map");
        ck(hipMalloc(reinterpret_cast<void **>(&roots_), n * 16), "hipMalloc ckks roots");
        ck(hipMalloc(reinterpret_cast<void **>(&inv_roots_), n * 16), "hipMalloc ckks roots");
        ck(hipMemcpy(inv_map_, inv.data(), n * 4, hipMemcpyHostToDevice), "upload ckks map");
        ck(hipMemcpy(roots_, rp.data(), n * 16, hipMemcpyHostToDevice), "upload ckks roots");
        ck(hipMemcpy(inv_roots_, irp.data(), n * 16, hipMemcpyHostToDevice), "upload ckks roots");
    }
    CKKSEncoder::~CKKSEncoder()
    {
        (void)hipFree(inv_map_);
        (void)hipFree(roots_);
        (void)hipFree(inv_roots_);
        for (auto &kv : consts_)
            (void)hipFree(kv.second.dev);
    }

    uint64_t *build_crt_constants(const Context &context, const Level &lvl)
    {
        const unsigned K = lvl.K;
        std::vector<uint64_t> q(context.coeff_modulus().begin(), context.coeff_modulus().begin() + K);
        std::vector<uint64_t> block((size_t)K * K + 2 * K + 2 * K, 0);
        for (unsigned j = 0; j < K; j++)
        {
            std::vector<uint64_t> others;
            for (unsigned i = 0; i < K; i++)
                if (i != j)
                    others.push_back(q[i]);
            std::vector<uint64_t> pp = others.empty() ? std::vector<uint64_t>{ 1 } : host::product(others);
            for (size_t w = 0; w < pp.size() && w < K; w++)
                block[(size_t)j * K + w] = pp[w];
            uint64_t pm = 1 % q[j];
            for (unsigned i = 0; i < K; i++)
                if (i != j)
                    pm = host::mulmod(pm, q[i] % q[j], q[j]);
            const ShoupOp ip = host::make_shoup(host::invmod(pm, q[j]), q[j]);
            block[(size_t)K * K + 2 * K + 2 * j] = ip.w;
            block[(size_t)K * K + 2 * K + 2 * j + 1] = ip.wq;
        }
        std::vector<uint64_t> Q = host::product(q);
        Q.resize(K, 0);
        // (Q + 1) >> 1
        std::vector<uint64_t> q1(K), half(K);
        uint64_t carry = 1;
        for (unsigned w = 0; w < K; w++)
        {
            q1[w] = Q[w] + carry;
            carry = (carry && q1[w] == 0) ? 1 : 0;
        }
        for (unsigned w = 0; w < K; w++)
            half[w] = (q1[w] >> 1) | (w + 1 < K ? q1[w + 1] << 63 : (carry << 63));
        for (unsigned w = 0; w < K; w++)
        {
            block[(size_t)K * K + w] = Q[w];
            block[(size_t)K * K + K + w] = half[w];
        }
        uint64_t *dev = nullptr;
        ck(hipMalloc(reinterpret_cast<void **>(&dev), block.size() * 8), "hipMalloc crt constants");
        ck(hipMemcpy(dev, block.data(), block.size() * 8, hipMemcpyHostToDevice), "upload crt constants");
        return dev;
    }

    const CKKSEncoder::LevelConst &CKKSEncoder::level_const(const Level &lvl) const
    {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = consts_.find(lvl.chain_index);
        if (it != consts_.end())
            return it->second;
        LevelConst lc;
        lc.dev = build_crt_constants(context_, lvl);
        lc.coeff_limit = coeff_limit(lvl.total_coeff_modulus_bit_count);
        return consts_.emplace(lvl.chain_index, lc).first->second;
    }

    unsigned CKKSEncoder::block_log() const
    {
        const unsigned n_log = (unsigned)context_.log_n();
        unsigned b = std::min(n_log, kFftLdsLog);
        // development builds only (SEALHIP_AB_SWITCHES): a smaller LDS block, so that the emulated tests reach the two-pass split
        // and every column-stage count at small N
        if (const char *e = shl_ab_getenv("SEALHIP_CKKS_FFT_BLOCK_LOG"))
            b = std::max<unsigned>(std::min<unsigned>((unsigned)std::atoi(e), b), std::max(1u, n_log > kFftMaxColumnLog ? n_log - kFftMaxColumnLog : 1u));
        return b;
    }
    size_t CKKSEncoder::chunk_items(size_t item_words) const
    {
        size_t budget = kCkksBatchScratchBytes;
        if (const char *e = shl_ab_getenv("SEALHIP_CKKS_SCRATCH_BYTES")) // development builds only: chunk edges at small N
            budget = (size_t)std::strtoull(e, nullptr, 10);
        const size_t items = item_words ? budget / (item_words * 8) : budget;
        return std::max<size_t>(1, std::min<size_t>(items, 65535)); // items are the grid's y dimension
    }
    static bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
    {
        const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
        return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
    }

    // encode_internal's argument checks, in its order (ckks.h:463-509)
    const Level &CKKSEncoder::encode_level(const uint64_t *parms_id, double scale, size_t value_count, bool have_values) const
    {
        const Level *lvl = parms_id ? context_.level_by_parms_id(parms_id) : nullptr;
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        if (!have_values && value_count > 0)
            throw std::invalid_argument("values cannot be null");
        if (value_count > slots_)
            throw std::invalid_argument("values_size is too large");
        if (!std::isnormal(scale) || scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= lvl->total_coeff_modulus_bit_count))
            throw std::invalid_argument("scale out of bounds");
        return *lvl;
    }
    // decode_internal's (ckks.h:686-716): a plaintext at a data level with a sane scale
    const Level &CKKSEncoder::decode_level(const uint64_t *parms_id, double scale) const
    {
        const Level *lvl = parms_id ? context_.level_by_parms_id(parms_id) : nullptr;
        if (!lvl || lvl->chain_index > context_.first_level().chain_index)
            throw std::invalid_argument("plain is not valid for encryption parameters");
        if (!std::isnormal(scale) || scale <= 0 || (static_cast<int>(std::log2(scale)) >= lvl->total_coeff_modulus_bit_count))
            throw std::invalid_argument("scale out of bounds");
        return *lvl;
    }

    void CKKSEncoder::encode_batch(const double *values, size_t value_count, size_t batch, bool is_complex, const Level &lvl, double scale,
                                   uint64_t *words) const
    {
        // ckks.h:510-680 for every item: placement + transform_from_rev + check + rounding / decomposition (k_ckks_encode), then
        // the forward NTT of every item's K residue polynomials
        const size_t n = context_.n(), K = lvl.K;
        const unsigned n_log = (unsigned)context_.log_n(), b = block_log();
        const LevelConst &lc = level_const(lvl);
        const bool two_pass = b < n_log;
        const size_t chunk = two_pass ? chunk_items(2 * n) : std::min<size_t>(batch, 65535);
        const size_t vstride = value_count * (is_complex ? 2 : 1);
        Scratch fail(1), mid(two_pass ? std::min(chunk, batch) * 2 * n : 1);
        ck(hipMemsetAsync(fail.p, 0, 8, nullptr), "zero failure word");
        for (size_t c0 = 0; c0 < batch; c0 += chunk)
        {
            const size_t items = std::min(chunk, batch - c0);
            CkksEncodeArgs a{};
            a.values = value_count ? values + c0 * vstride : nullptr;
            a.value_count = value_count;
            a.is_complex = is_complex;
            a.inv_map = inv_map_;
            a.inv_roots = inv_roots_;
            a.mods = context_.dev_mods();
            a.K = (unsigned)K;
            a.fix = scale / static_cast<double>(n);
            a.coeff_limit = lc.coeff_limit;
            a.words = words + c0 * K * n;
            a.mid = reinterpret_cast<double2 *>(mid.p);
            a.fail = reinterpret_cast<unsigned *>(fail.p);
            a.item0 = (unsigned)c0;
            a.n_log = n_log;
            a.block_log = b;
            ck(k_ckks_encode(a, (unsigned)items, nullptr), "ckks encode");
            ck(ntt_forward(context_.ntt_tables(), plain_batch(a.words, K * n, (unsigned)K, (unsigned)items, 0), 0, nullptr), "ntt plaintexts");
        }
        unsigned f = 0;
        ck(hipMemcpy(&f, fail.p, 4, hipMemcpyDeviceToHost), "encode sync");
        if (f)
        {
            const unsigned code = ~f;
            throw std::invalid_argument(std::string(code & 1 ? "encoded values are too large" : "values must be finite") + " (item " +
                                        std::to_string(code >> 1) + ")");
        }
    }

    void CKKSEncoder::encode(const double *values, size_t count, bool is_complex, const uint64_t *parms_id, double scale, Plaintext &dest) const
    {
        // ckks.h:458-680: a batch of one
        if (&dest.context() != &context_)
            throw std::invalid_argument("destination belongs to another context");
        const Level &lvl = encode_level(parms_id, scale, count, values != nullptr);
        const size_t n = context_.n(), K = lvl.K, vw = count * (is_complex ? 2 : 1);
        Scratch vin(vw ? vw : 1);
        if (vw)
            ck(hipMemcpy(vin.p, values, vw * 8, hipMemcpyHostToDevice), "upload values");
        uint64_t *slab = DevicePool::global().alloc_words(K * n);
        try
        {
            encode_batch(reinterpret_cast<const double *>(vin.p), count, 1, is_complex, lvl, scale, slab);
        }
        catch (...)
        {
            DevicePool::global().free_words(slab);
            throw;
        }
        dest.adopt(slab, K * n, K * n);
        dest.set_level(&lvl);
        dest.scale() = scale;
    }
    void CKKSEncoder::encode_device(const double *values, size_t value_count, size_t batch, bool is_complex, const uint64_t *parms_id, double scale,
                                    uint64_t *words) const
    {
        const Level &lvl = encode_level(parms_id, scale, value_count, values != nullptr || !batch);
        if (!batch)
            return;
        if (!words)
            throw std::invalid_argument("destination cannot be null");
        if (overlap(values, batch * value_count * (is_complex ? 16 : 8), words, batch * lvl.K * context_.n() * 8))
            throw std::invalid_argument("values and destination overlap");
        encode_batch(values, value_count, batch, is_complex, lvl, scale, words);
    }

    void CKKSEncoder::fill_constant(const Level &lvl, const std::vector<uint64_t> &residues, double scale, Plaintext &dest) const
    {
        if (&dest.context() != &context_)
            throw std::invalid_argument("destination belongs to another context");
        const size_t n = context_.n(), K = lvl.K;
        std::vector<uint64_t> words(K * n);
        for (size_t j = 0; j < K; j++)
            std::fill_n(words.begin() + j * n, n, residues[j]);
        uint64_t *slab = DevicePool::global().alloc_words(K * n);
        hipError_t e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess)
            e = hipMemcpy(slab, words.data(), K * n * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess)
        {
            DevicePool::global().free_words(slab);
            ck(e, "upload constant plaintext");
        }
        dest.adopt(slab, K * n, K * n);
        dest.set_level(&lvl);
        dest.scale() = scale;
    }
    // the level and the scale check of encode(double) (ckks.cpp:72-90)
    const Level &CKKSEncoder::value_level(const uint64_t *parms_id, double scale) const
    {
        const Level *lvl = parms_id ? context_.level_by_parms_id(parms_id) : nullptr;
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        if (!std::isfinite(scale) || scale <= 0 || (static_cast<int>(std::log2(scale)) >= lvl->total_coeff_modulus_bit_count))
            throw std::invalid_argument("scale out of bounds");
        return *lvl;
    }
    // encode(double) without the fill (ckks.cpp:91-205): the value's checks, then the K words every coefficient of the constant
    // plaintext holds.  Host doubles and the host libm on purpose: branch and range checks go through log2
    void CKKSEncoder::value_residues(double value, const Level &lvl, double scale, uint64_t *residues) const
    {
        if (!std::isfinite(value))
            throw std::invalid_argument("value must be finite");
        value *= scale;
        if (!std::isfinite(value))
            throw std::invalid_argument("encoded value is too large");
        const int coeff_bit_count = (std::fabs(value) < 1.0) ? 2 : (static_cast<int>(std::log2(std::fabs(value))) + 2);
        if (coeff_bit_count >= lvl.total_coeff_modulus_bit_count)
            throw std::invalid_argument("encoded value is too large");
        const double two_pow_64 = std::pow(2.0, 64);
        double coeffd = std::round(value);
        const bool is_negative = std::signbit(coeffd);
        coeffd = std::fabs(coeffd);
        for (unsigned j = 0; j < lvl.K; j++)
        {
            const uint64_t q = context_.coeff_modulus()[j];
            uint64_t r;
            if (coeff_bit_count <= 64)
                r = static_cast<uint64_t>(std::fabs(coeffd)) % q;
            else if (coeff_bit_count > 128)
            {
                // ckks.cpp:165-196: the double cut into 64-bit words (fmod / division by 2^64, exact), reduced modulo q
                // (RNSBase::decompose); Horner from the top word
                std::vector<uint64_t> words;
                for (double c = coeffd; c >= 1 && words.size() < lvl.K; c /= two_pow_64)
                    words.push_back(static_cast<uint64_t>(std::fmod(c, two_pow_64)));
                unsigned __int128 acc = 0;
                for (size_t w = words.size(); w-- > 0;)
                    acc = ((acc << 64) | words[w]) % q;
                r = (uint64_t)acc;
            }
            else
            {
                const unsigned __int128 v = ((unsigned __int128) static_cast<uint64_t>(coeffd / two_pow_64) << 64) |
                                            static_cast<uint64_t>(std::fmod(coeffd, two_pow_64));
                r = (uint64_t)(v % q);
            }
            residues[j] = is_negative ? (r ? q - r : 0) : r;
        }
    }
    // encode(int64_t) without the fill (ckks.cpp:207-250)
    void CKKSEncoder::integer_residues(int64_t value, const Level &lvl, uint64_t *residues) const
    {
        const uint64_t mag = value < 0 ? (uint64_t)0 - (uint64_t)value : (uint64_t)value;
        const int coeff_bit_count = (mag ? 64 - __builtin_clzll(mag) : 0) + 2;
        if (coeff_bit_count >= lvl.total_coeff_modulus_bit_count)
            throw std::invalid_argument("encoded value is too large");
        for (unsigned j = 0; j < lvl.K; j++)
        {
            const uint64_t q = context_.coeff_modulus()[j];
            uint64_t tmp = static_cast<uint64_t>(value);
            if (value < 0)
                tmp += q; // wraps modulo 2^64, as the reference's line does
            residues[j] = tmp % q;
        }
    }
    void CKKSEncoder::encode_value(double value, const uint64_t *parms_id, double scale, Plaintext &dest) const
    {
        // ckks.cpp:72-205
        const Level &lvl = value_level(parms_id, scale);
        std::vector<uint64_t> residues(lvl.K);
        value_residues(value, lvl, scale, residues.data());
        fill_constant(lvl, residues, scale, dest);
    }
    void CKKSEncoder::encode_integer(int64_t value, const uint64_t *parms_id, Plaintext &dest) const
    {
        // ckks.cpp:207-250
        const Level *lvl = parms_id ? context_.level_by_parms_id(parms_id) : nullptr;
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        std::vector<uint64_t> residues(lvl->K);
        integer_residues(value, *lvl, residues.data());
        fill_constant(*lvl, residues, 1.0, dest);
    }

    // `count` scalar plaintexts as [count][K] words in device memory (include/sealhip.h: CKKSEncoder_EncodeScalars): residues(i, out)
    // gives scalar i's K words or throws the per-object form's refusal, which is passed on with the index.  Nothing is written
    // unless every value passes; then one synchronous copy after a drain (not a hot-path call, like ItemMap_Create)
    template <class Residues>
    void CKKSEncoder::upload_scalars(size_t count, const void *values, const Level &lvl, uint64_t *words, Residues residues) const
    {
        if (!count)
            throw std::invalid_argument("count cannot be zero");
        if (!values || !words)
            throw std::invalid_argument(values ? "device_words cannot be null" : "values cannot be null");
        if ((uintptr_t)words % 16)
            throw std::invalid_argument("device_words must be 16-byte aligned");
        std::vector<uint64_t> host(count * lvl.K);
        for (size_t i = 0; i < count; i++)
        {
            try
            {
                residues(i, host.data() + i * lvl.K);
            }
            catch (const std::invalid_argument &e)
            {
                throw std::invalid_argument(std::string(e.what()) + " (values[" + std::to_string(i) + "])");
            }
        }
        ck(hipDeviceSynchronize(), "scalars upload"); // whatever read or wrote the buffer before is done
        copy_h2d(words, host.data(), host.size() * 8);
    }
    void CKKSEncoder::encode_scalars(size_t count, const double *values, const uint64_t *parms_id, double scale, uint64_t *words) const
    {
        const Level &lvl = value_level(parms_id, scale);
        upload_scalars(count, values, lvl, words, [&](size_t i, uint64_t *out) { value_residues(values[i], lvl, scale, out); });
    }
    void CKKSEncoder::encode_integer_scalars(size_t count, const int64_t *values, const uint64_t *parms_id, uint64_t *words) const
    {
        const Level *lvl = parms_id ? context_.level_by_parms_id(parms_id) : nullptr;
        if (!lvl)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        upload_scalars(count, values, *lvl, words, [&](size_t i, uint64_t *out) { integer_residues(values[i], *lvl, out); });
    }

    void CKKSEncoder::decode_batch(const uint64_t *words, size_t batch, const Level &lvl, double scale, bool want_complex, double *values) const
    {
        // ckks.h:717-789 for every item: the inverse NTT on a copy, then CRT composition + scaling + transform_to_rev + the slot
        // gather (k_ckks_decode)
        const size_t n = context_.n(), K = lvl.K;
        const unsigned n_log = (unsigned)context_.log_n(), b = block_log();
        const LevelConst &lc = level_const(lvl);
        const bool two_pass = b < n_log;
        const size_t chunk = chunk_items(K * n + (two_pass ? 2 * n : 0));
        const size_t first = std::min(chunk, batch);
        Scratch copy(first * K * n), mid(two_pass ? first * 2 * n : 1);
        for (size_t c0 = 0; c0 < batch; c0 += chunk)
        {
            const size_t items = std::min(chunk, batch - c0);
            ck(hipMemcpyAsync(copy.p, words + c0 * K * n, items * K * n * 8, hipMemcpyDeviceToDevice, nullptr), "copy words");
            ck(ntt_inverse(context_.ntt_tables(), plain_batch(copy.p, K * n, (unsigned)K, (unsigned)items, 0), 0, nullptr), "intt plaintexts");
            CkksDecodeArgs a{};
            a.residues = copy.p;
            a.mods = context_.dev_mods();
            a.punct = lc.dev;
            a.inv_punct = reinterpret_cast<const ShoupOp *>(lc.dev + K * K + 2 * K);
            a.q_words = lc.dev + K * K;
            a.half_words = lc.dev + K * K + K;
            a.inv_scale = double(1.0) / scale;
            a.inv_map = inv_map_;
            a.roots = roots_;
            a.mid = reinterpret_cast<double2 *>(mid.p);
            a.out = values + c0 * slots_ * (want_complex ? 2 : 1);
            a.want_complex = want_complex;
            a.K = (unsigned)K;
            a.n_log = n_log;
            a.block_log = b;
            ck(k_ckks_decode(a, (unsigned)items, nullptr), "ckks decode");
        }
        ck(hipStreamSynchronize(nullptr), "decode sync"); // the scratch goes back to the pool
    }

    void CKKSEncoder::decode(const Plaintext &plain, double *values, bool want_complex) const
    {
        // ckks.h:683-789: a batch of one
        if (&plain.context() != &context_ || (plain.is_ntt_form() && plain.coeff_count() != plain.level()->K * context_.n()))
            throw std::invalid_argument("plain is not valid for encryption parameters");
        if (!plain.is_ntt_form())
            throw std::invalid_argument("plain is not in NTT form");
        if (!values)
            throw std::invalid_argument("destination cannot be null");
        const Level &lvl = decode_level(plain.level()->parms_id, plain.scale());
        const size_t words = slots_ * (want_complex ? 2 : 1);
        Scratch out(words);
        decode_batch(plain.data(), 1, lvl, plain.scale(), want_complex, reinterpret_cast<double *>(out.p));
        ck(hipMemcpy(values, out.p, words * 8, hipMemcpyDeviceToHost), "download values");
    }
    void CKKSEncoder::decode_device(const uint64_t *words, size_t batch, const uint64_t *parms_id, double scale, bool want_complex,
                                    double *values) const
    {
        const Level &lvl = decode_level(parms_id, scale);
        if (!batch)
            return;
        if (!words || !values)
            throw std::invalid_argument(words ? "destination cannot be null" : "plain cannot be null");
        if (overlap(words, batch * lvl.K * context_.n() * 8, values, batch * slots_ * (want_complex ? 16 : 8)))
            throw std::invalid_argument("plain and destination overlap");
        decode_batch(words, batch, lvl, scale, want_complex, values);
    }
} // namespace sealhip
