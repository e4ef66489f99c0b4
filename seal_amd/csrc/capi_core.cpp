// extern "C" layer, part 1: library / device, parameter helpers, SEALContext, Ciphertext and Plaintext objects, wire format (include/sealhip.h)
#include "capi_common.h"
#include <memory>

namespace sealhip
{
    std::string &capi_last_error()
    {
        thread_local std::string message;
        return message;
    }
}

namespace
{
    void require_device()
    {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            throw std::runtime_error("no HIP device visible: libsealhip has no CPU fallback");
    }
    const Level &level_at(const Context &c, uint64_t chain_index)
    {
        const Level *l = c.level_by_chain_index(chain_index);
        if (!l)
            throw std::out_of_range("chain_index");
        return *l;
    }
    // a getter of one Ciphertext property
    template <class T, class Get>
    SHL_HRESULT ct_get(void *thisptr, T *out, Get get)
    {
        return guarded({ thisptr, out }, [&] { *out = get(*as<Ciphertext>(thisptr)); });
    }
    size_t ct_raw_bytes(const Ciphertext &ct)
    {
        return serial::ciphertext_save_size(ct.size(), ct.poly_modulus_degree(), ct.coeff_modulus_size());
    }
    void check_slab(const Ciphertext &ct, uint64_t word_count)
    {
        if (word_count != ct.word_count())
            throw std::invalid_argument("word_count does not match the ciphertext slab");
    }
} // namespace

extern "C"
{
    // ------------------------------------------------------------------ library / device
    SHL_FUNC SealHip_Version(uint32_t *major, uint32_t *minor, uint32_t *patch)
    {
        return guarded({ major, minor, patch }, [&] {
            *major = 0;
            *minor = 1;
            *patch = 0;
        });
    }
    SHL_FUNC SealHip_DeviceInfo(char *name, uint64_t name_capacity, int *compute_units, uint64_t *hbm_bytes)
    {
        return guarded({}, [&] {
            require_device();
            int dev = 0;
            hip_ok(hipGetDevice(&dev), "hipGetDevice");
            hipDeviceProp_t prop;
            hip_ok(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
            if (name && name_capacity)
            {
                std::strncpy(name, prop.name, name_capacity - 1);
                name[name_capacity - 1] = 0;
            }
            if (compute_units)
                *compute_units = prop.multiProcessorCount;
            if (hbm_bytes)
                *hbm_bytes = prop.totalGlobalMem;
        });
    }
    SHL_FUNC SealHip_LastError(char *outstr, uint64_t *length)
    {
        return guarded({ length }, [&] {
            const std::string &message = sealhip::capi_last_error();
            if (outstr && *length > message.size())
                std::memcpy(outstr, message.c_str(), message.size() + 1);
            *length = message.size() + 1;
        });
    }

    // ------------------------------------------------------------------ parameter helpers
    SHL_FUNC CoeffModulus_Create1(uint64_t poly_modulus_degree, uint64_t length, int *bit_sizes, uint64_t *coeffs)
    {
        return guarded({ bit_sizes, coeffs }, [&] {
            if (poly_modulus_degree < 2 || poly_modulus_degree > 131072 || (poly_modulus_degree & (poly_modulus_degree - 1)))
                throw std::invalid_argument("poly_modulus_degree is invalid");
            std::vector<int> bits(bit_sizes, bit_sizes + length);
            auto v = host::coeff_modulus_create(poly_modulus_degree, bits);
            for (size_t i = 0; i < v.size(); i++)
                coeffs[i] = v[i];
        });
    }
    SHL_FUNC PlainModulus_Batching(uint64_t poly_modulus_degree, int bit_size, uint64_t *value)
    {
        return guarded({ value }, [&] { *value = host::plain_modulus_batching(poly_modulus_degree, bit_size); });
    }

    SHL_FUNC EncParams_Create1(uint8_t scheme, void **enc_params)
    {
        return guarded({ enc_params }, [&] {
            if (scheme > 3)
                throw std::invalid_argument("unsupported scheme");
            auto p = new EncParams();
            p->scheme = scheme;
            *enc_params = p;
        });
    }
    SHL_FUNC EncParams_Destroy(void *thisptr)
    {
        return guarded({ thisptr }, [&] { delete as<EncParams>(thisptr); });
    }
    SHL_FUNC EncParams_SetPolyModulusDegree(void *thisptr, uint64_t degree)
    {
        return guarded({ thisptr }, [&] { as<EncParams>(thisptr)->n = degree; });
    }
    SHL_FUNC EncParams_GetPolyModulusDegree(void *thisptr, uint64_t *degree)
    {
        return guarded({ thisptr, degree }, [&] { *degree = as<EncParams>(thisptr)->n; });
    }
    SHL_FUNC EncParams_SetCoeffModulus(void *thisptr, uint64_t length, const uint64_t *coeffs)
    {
        return guarded({ thisptr, coeffs }, [&] {
            if (length < 1 || length > kMaxComps)
                throw std::invalid_argument("coeff_modulus is invalid");
            as<EncParams>(thisptr)->coeff_modulus.assign(coeffs, coeffs + length);
        });
    }
    SHL_FUNC EncParams_GetCoeffModulus(void *thisptr, uint64_t *length, uint64_t *coeffs)
    {
        return guarded({ thisptr, length }, [&] {
            auto &v = as<EncParams>(thisptr)->coeff_modulus;
            *length = v.size();
            if (coeffs)
                std::memcpy(coeffs, v.data(), v.size() * 8);
        });
    }
    SHL_FUNC EncParams_SetPlainModulus2(void *thisptr, uint64_t plain_modulus)
    {
        return guarded({ thisptr }, [&] {
            auto p = as<EncParams>(thisptr);
            // EncryptionParameters::set_plain_modulus (encryptionparams.h): CKKS takes none
            if (p->scheme == 2 && plain_modulus != 0)
                throw std::logic_error("plain_modulus is not supported for this scheme");
            p->plain_modulus = plain_modulus;
        });
    }
    SHL_FUNC EncParams_GetScheme(void *thisptr, uint8_t *scheme)
    {
        return guarded({ thisptr, scheme }, [&] { *scheme = as<EncParams>(thisptr)->scheme; });
    }

    // ------------------------------------------------------------------ SEALContext
    SHL_FUNC SEALContext_Create(void *encryptionParams, bool expand_mod_chain, int sec_level, void **context)
    {
        return guarded({ encryptionParams, context }, [&] {
            require_device();
            auto p = as<EncParams>(encryptionParams);
            // sec_level_type (0 none, 128, 192, 256): the reference marks parameters whose total coefficient modulus exceeds
            // CoeffModulus::MaxBitCount(N, sec_level) (util/hestdparms.h:19-80; 0 for degrees the standard does not list) as
            // invalid_parameters_insecure (context.cpp:219-231) and every later use throws; here the context is refused
            int max_bits = 0;
            if (sec_level != 0)
            {
                static const int table[3][6] = { { 27, 54, 109, 218, 438, 881 }, { 19, 37, 75, 152, 305, 611 }, { 14, 29, 58, 118, 237, 476 } };
                const int row = sec_level == 128 ? 0 : sec_level == 192 ? 1 : sec_level == 256 ? 2 : -1;
                if (row < 0)
                    throw std::invalid_argument("invalid security level");
                for (int i = 0; i < 6; i++)
                    if (p->n == (uint64_t(1024) << i))
                        max_bits = table[row][i];
            }
            // ... before any device table is built: the verdict follows from the primes alone - but behind the checks the
            // reference makes first, so that malformed AND oversized parameters report the malformation
            Context::check_basic_parameters(static_cast<Scheme>(p->scheme), p->n, p->coeff_modulus);
            if (sec_level != 0 && !p->coeff_modulus.empty() && host::significant_bits(host::product(p->coeff_modulus)) > max_bits)
                throw std::invalid_argument("encryption parameters are not set correctly: not secure for the requested security level");
            std::unique_ptr<Context> c(new Context(static_cast<Scheme>(p->scheme), p->n, p->coeff_modulus, p->plain_modulus, expand_mod_chain));
            if (sec_level != 0 && c->key_level().total_coeff_modulus_bit_count > max_bits)
                throw std::invalid_argument("encryption parameters are not set correctly: not secure for the requested security level");
            c->set_sec_level(sec_level);
            *context = c.release();
        });
    }
    SHL_FUNC SEALContext_Destroy(void *thisptr)
    {
        return guarded({ thisptr }, [&] {
            sealhip::capi_forget_context(as<Context>(thisptr));
            delete as<Context>(thisptr);
        });
    }
    SHL_FUNC SEALContext_KeyParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, &as<Context>(thisptr)->key_level()); });
    }
    SHL_FUNC SEALContext_FirstParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, &as<Context>(thisptr)->first_level()); });
    }
    SHL_FUNC SEALContext_LastParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, &as<Context>(thisptr)->last_level()); });
    }
    SHL_FUNC SEALContext_UsingKeyswitching(void *thisptr, bool *using_keyswitching)
    {
        return guarded({ thisptr, using_keyswitching }, [&] { *using_keyswitching = as<Context>(thisptr)->using_keyswitching(); });
    }
    SHL_FUNC SEALContext_ChainIndex(void *thisptr, uint64_t *parms_id, uint64_t *chain_index)
    {
        return guarded({ thisptr, parms_id, chain_index }, [&] {
            auto l = as<Context>(thisptr)->level_by_parms_id(parms_id);
            if (!l)
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            *chain_index = l->chain_index;
        });
    }
    SHL_FUNC SEALContext_ParmsIdAt(void *thisptr, uint64_t chain_index, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, &level_at(*as<Context>(thisptr), chain_index)); });
    }
    SHL_FUNC SEALContext_CoeffModulusAt(void *thisptr, uint64_t chain_index, uint64_t *length, uint64_t *coeffs)
    {
        return guarded({ thisptr, length }, [&] {
            auto c = as<Context>(thisptr);
            *length = level_at(*c, chain_index).K;
            if (coeffs)
                std::memcpy(coeffs, c->coeff_modulus().data(), *length * 8);
        });
    }
    SHL_FUNC SEALContext_TotalCoeffModulusBitCount(void *thisptr, uint64_t chain_index, int *bit_count)
    {
        return guarded({ thisptr, bit_count }, [&] { *bit_count = level_at(*as<Context>(thisptr), chain_index).total_coeff_modulus_bit_count; });
    }
    SHL_FUNC SEALContext_SetParmsId(void *thisptr, uint64_t chain_index, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] {
            level_at(*as<Context>(thisptr), chain_index);
            as<Context>(thisptr)->set_parms_id(chain_index, parms_id);
        });
    }
    SHL_FUNC SEALContext_NTTRoot(void *thisptr, uint64_t prime_index, uint64_t *root)
    {
        return guarded({ thisptr, root }, [&] {
            auto c = as<Context>(thisptr);
            if (prime_index >= c->pool_primes().size())
                throw std::out_of_range("prime_index");
            *root = c->ntt_root((unsigned)prime_index);
        });
    }
    SHL_FUNC SEALContext_BaseBsk(void *thisptr, uint64_t chain_index, uint64_t *length, uint64_t *primes)
    {
        return guarded({ thisptr, length }, [&] {
            const Level &l = level_at(*as<Context>(thisptr), chain_index);
            *length = l.bsk.size();
            if (primes)
                std::memcpy(primes, l.bsk.data(), l.bsk.size() * 8);
        });
    }

    // ------------------------------------------------------------------ Ciphertext
    SHL_FUNC Ciphertext_Create3(void *context, void *pool, void **cipher)
    {
        (void)pool;
        return guarded({ context, cipher }, [&] { *cipher = new Ciphertext(*as<Context>(context), 1); });
    }
    SHL_FUNC Ciphertext_CreateBatch(void *context, uint64_t batch, void **cipher)
    {
        return guarded({ context, cipher }, [&] {
            if (batch == 0)
                throw std::invalid_argument("batch must be positive");
            *cipher = new Ciphertext(*as<Context>(context), batch);
        });
    }
    SHL_FUNC Ciphertext_Create2(void *copy, void **cipher)
    {
        return guarded({ copy, cipher }, [&] {
            hip_ok(hipDeviceSynchronize(), "sync");
            *cipher = new Ciphertext(*as<Ciphertext>(copy));
            hip_ok(hipDeviceSynchronize(), "sync");
        });
    }
    SHL_FUNC Ciphertext_Set(void *thisptr, void *assign)
    {
        return guarded({ thisptr, assign }, [&] {
            hip_ok(hipDeviceSynchronize(), "sync");
            *as<Ciphertext>(thisptr) = *as<Ciphertext>(assign);
            hip_ok(hipDeviceSynchronize(), "sync");
        });
    }
    SHL_FUNC Ciphertext_Destroy(void *thisptr)
    {
        return guarded({ thisptr }, [&] { delete as<Ciphertext>(thisptr); });
    }
    SHL_FUNC Ciphertext_Resize1(void *thisptr, void *context, uint64_t *parms_id, uint64_t size)
    {
        return guarded({ thisptr, context, parms_id }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            auto c = as<Context>(context);
            if (&ct->context() != c)
                throw std::invalid_argument("ciphertext belongs to another context");
            hip_ok(hipDeviceSynchronize(), "sync"); // the copy / zero fill below run on the NULL stream: nothing queued elsewhere may still touch the words
            ct->resize(c->level_by_parms_id(parms_id), size, nullptr);
        });
    }
    SHL_FUNC Ciphertext_Size(void *thisptr, uint64_t *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.size(); });
    }
    SHL_FUNC Ciphertext_BatchCount(void *thisptr, uint64_t *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.batch(); });
    }
    SHL_FUNC Ciphertext_PolyModulusDegree(void *thisptr, uint64_t *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.poly_modulus_degree(); });
    }
    SHL_FUNC Ciphertext_CoeffModulusSize(void *thisptr, uint64_t *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.coeff_modulus_size(); });
    }
    SHL_FUNC Ciphertext_IsNTTForm(void *thisptr, bool *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.is_ntt_form(); });
    }
    SHL_FUNC Ciphertext_Scale(void *thisptr, double *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.scale(); });
    }
    SHL_FUNC Ciphertext_CorrectionFactor(void *thisptr, uint64_t *out)
    {
        return ct_get(thisptr, out, [](Ciphertext &ct) { return ct.correction_factor(); });
    }
    SHL_FUNC Ciphertext_ParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, as<Ciphertext>(thisptr)->level()); });
    }
    SHL_FUNC Ciphertext_SetIsNTTForm(void *thisptr, bool is_ntt_form)
    {
        return guarded({ thisptr }, [&] { as<Ciphertext>(thisptr)->is_ntt_form() = is_ntt_form; });
    }
    SHL_FUNC Ciphertext_SetScale(void *thisptr, double scale)
    {
        return guarded({ thisptr }, [&] { as<Ciphertext>(thisptr)->scale() = scale; });
    }
    SHL_FUNC Ciphertext_SetCorrectionFactor(void *thisptr, uint64_t correction_factor)
    {
        return guarded({ thisptr }, [&] { as<Ciphertext>(thisptr)->correction_factor() = correction_factor; });
    }
    SHL_FUNC Ciphertext_IsTransparent(void *thisptr, bool *result)
    {
        return guarded({ thisptr, result }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            Evaluator ev(ct->context());
            hip_ok(hipDeviceSynchronize(), "sync");
            *result = ev.is_transparent(*ct);
        });
    }
    SHL_FUNC Ciphertext_DevicePtr(void *thisptr, uint64_t **data, uint64_t *word_count)
    {
        // data() completes a pending key-switch tail: kernel launches, a pool allocation - it can throw
        return guarded({ thisptr, data }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            *data = ct->data();
            if (word_count)
                *word_count = ct->word_count();
        });
    }
    SHL_FUNC Ciphertext_CopyFromHost(void *thisptr, const uint64_t *src, uint64_t word_count)
    {
        return guarded({ thisptr, src }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            check_slab(*ct, word_count);
            hip_ok(hipDeviceSynchronize(), "sync");
            copy_h2d(ct->data(), src, word_count * 8);
        });
    }
    SHL_FUNC Ciphertext_CopyToHost(void *thisptr, uint64_t *dst, uint64_t word_count)
    {
        return guarded({ thisptr, dst }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            check_slab(*ct, word_count);
            hip_ok(hipDeviceSynchronize(), "sync");
            copy_d2h(dst, ct->data(), word_count * 8);
        });
    }
    SHL_FUNC Ciphertext_CopyWordsToHost(void *thisptr, uint64_t word_offset, uint64_t word_count, uint64_t *dst)
    {
        return guarded({ thisptr, dst }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            if (word_offset > ct->word_count() || word_count > ct->word_count() - word_offset)
                throw std::invalid_argument("word range outside the ciphertext slab");
            hip_ok(hipDeviceSynchronize(), "sync");
            if (word_count)
                copy_d2h(dst, ct->data() + word_offset, word_count * 8);
        });
    }
    SHL_FUNC Ciphertext_CopyFromDevice(void *thisptr, const uint64_t *src, uint64_t word_count, void *hip_stream)
    {
        return guarded({ thisptr, src }, [&] {
            auto ct = as<Ciphertext>(thisptr);
            check_slab(*ct, word_count);
            hip_ok(hipMemcpyAsync(ct->data(), src, word_count * 8, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream), "D2D");
        });
    }

    // ---- wire format (native/src/seal/c/ciphertext.h:80-86; seal_amd/csrc/serial.h)
    namespace
    {
        // one host image -> batch slot `item` of a device-resident batch.  set_meta: the image defines the batch's metadata
        // (first item / batch of one); otherwise it has to agree with the items already there.
        void upload_image(Ciphertext &ct, const Context &c, serial::CiphertextImage &img, size_t item, bool set_meta)
        {
            if (&ct.context() != &c)
                throw std::invalid_argument("ciphertext belongs to another context");
            if (item >= ct.batch())
                throw std::out_of_range("batch item");
            // BGV ciphertexts are serialized in coefficient form and transformed on load (ciphertext.cpp:384-403)
            const bool to_ntt = c.scheme() == Scheme::bgv && !img.is_ntt_form && img.word_count() != 0;
            const bool ntt_form = img.is_ntt_form || to_ntt;
            hip_ok(hipDeviceSynchronize(), "sync");
            if (set_meta)
            {
                ct.resize(img.level, (size_t)img.size, nullptr);
                ct.is_ntt_form() = ntt_form;
                ct.scale() = img.scale;
                ct.correction_factor() = img.correction_factor;
            }
            else if (ct.level() != img.level || ct.size() != img.size || ct.is_ntt_form() != ntt_form || ct.scale() != img.scale ||
                     ct.correction_factor() != img.correction_factor)
                throw std::invalid_argument("serialized ciphertext does not match the metadata of the batch");
            if (img.word_count() == 0)
                return;
            const size_t n = c.n(), K = img.level->K, poly_words = K * n;
            uint64_t *tmp = nullptr;
            hip_ok(hipMalloc(reinterpret_cast<void **>(&tmp), img.word_count() * 8), "hipMalloc");
            // the stored piece goes to the device straight from the caller's stream buffer
            hipError_t e = img.stored_words ? hipMemcpy(tmp, img.stored, img.stored_words * 8, hipMemcpyHostToDevice) : hipSuccess;
            if (e == hipSuccess && !img.expanded.empty())
                e = hipMemcpy(tmp + img.stored_words, img.expanded.data(), img.expanded.size() * 8, hipMemcpyHostToDevice);
            if (e == hipSuccess && img.pending_words)
            {
                // the seeded c_1: sample_poly_uniform over Blake2xb on the device (xof.h)
                try
                {
                    sample_uniform_device(c, K, { seeded_piece(img, tmp) });
                }
                catch (...)
                {
                    (void)hipFree(tmp);
                    throw;
                }
            }
            if (e == hipSuccess && to_ntt)
            {
                e = ntt_forward(c.ntt_tables(), plain_batch(tmp, poly_words, (unsigned)K, (unsigned)img.size, 0), 0, nullptr);
            }
            for (size_t p = 0; e == hipSuccess && p < img.size; p++)
                e = hipMemcpyAsync(ct.plane(p) + item * poly_words, tmp + p * poly_words, poly_words * 8, hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess)
                e = hipDeviceSynchronize();
            (void)hipFree(tmp);
            hip_ok(e, "ciphertext upload");
        }
        SHL_HRESULT ct_load(void *thisptr, void *context, uint64_t item, bool whole, uint8_t *inptr, uint64_t size, int64_t *in_bytes, bool check)
        {
            return load_stream<Ciphertext>(thisptr, context, inptr, in_bytes, [&](Ciphertext &ct, Context &c) {
                if (whole && ct.batch() != 1)
                    throw std::invalid_argument("Ciphertext_Load needs a batch of one: use Ciphertext_LoadItem for a slot of a batch");
                serial::CiphertextImage img;
                const size_t bytes = serial::load_ciphertext(c, inptr, (size_t)size, check, img, true);
                // the first item loaded into an empty batch defines its metadata
                upload_image(ct, c, img, (size_t)item, whole || ct.size() == 0);
                return bytes;
            });
        }
        SHL_HRESULT ks_load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes, bool check)
        {
            return load_stream<KSwitchKeys>(thisptr, context, inptr, in_bytes, [&](KSwitchKeys &keys, Context &c) {
                serial::KSwitchKeysImage img;
                const size_t bytes = serial::load_kswitchkeys(c, inptr, (size_t)size, check, img, true);
                keys.clear(); // the loaded object replaces the previous contents, indices absent from the stream included
                keys.reserve_slots(img.keys.size());
                for (size_t index = 0; index < img.keys.size(); index++)
                {
                    auto &digits = img.keys[index];
                    if (digits.empty())
                        continue;
                    // [digit][2][L][N], the layout of KSwitchKeys::keys_[index][digit].data() (kswitchkeys.h:340); every piece is
                    // copied to the device from where it lies (the stream buffer / the expanded c_1): no host staging copy
                    keys.set_key_with(c, index, digits.size(), [&](uint64_t *dst) {
                        std::vector<XofJob> seeded; // the c_1 halves a Blake2xb seed stands for: expanded on the device, all digits at once
                        for (auto &d : digits)
                        {
                            if (d.stored_words)
                                hip_ok(hipMemcpy(dst, d.stored, d.stored_words * 8, hipMemcpyHostToDevice), "upload key");
                            if (!d.expanded.empty())
                                hip_ok(hipMemcpy(dst + d.stored_words, d.expanded.data(), d.expanded.size() * 8, hipMemcpyHostToDevice), "upload key");
                            if (d.pending_words)
                                seeded.push_back(seeded_piece(d, dst));
                            dst += d.word_count();
                        }
                        sample_uniform_device(c, c.key_level().K, seeded);
                    });
                    for (auto &d : digits)
                        std::vector<uint64_t>().swap(d.expanded);
                }
                return bytes;
            });
        }
        SHL_HRESULT pt_load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes, bool check)
        {
            return load_stream<Plaintext>(thisptr, context, inptr, in_bytes, [&](Plaintext &pt, Context &c) {
                if (&pt.context() != &c)
                    throw std::invalid_argument("plaintext belongs to another context");
                serial::PlaintextImage img;
                const size_t bytes = serial::load_plaintext(c, inptr, (size_t)size, check, img);
                hip_ok(hipDeviceSynchronize(), "sync");
                pt.set(reinterpret_cast<const uint64_t *>(img.stored), (size_t)img.coeff_count, false); // H2D straight from the stream
                pt.set_level(img.level);
                pt.scale() = img.scale;
                return bytes;
            });
        }
        // KSwitchKeys::save_members (kswitchkeys.cpp:47-90): parms_id, the slot count, per slot the digit count and every digit as
        // the stream of its (full, size-2, key-level, NTT-form) ciphertext - the whole inside one SEALHeader
        size_t ks_raw_size(const KSwitchKeys &keys)
        {
            size_t bytes = 16 + 32 + 8 + 8 * keys.slots();
            if (const Context *c = keys.context())
                for (size_t i = 0; i < keys.slots(); i++)
                    if (keys.has_key(i))
                    {
                        // (a size for a stream that cannot be written would be a trap)
                        if (keys.key(i).digit0 != 0 || keys.key(i).digits != c->first_level().K)
                            throw std::logic_error("a digit-parallel slice of a key cannot be saved");
                        bytes += keys.key(i).digits * serial::ciphertext_save_size(2, c->n(), c->key_level().K);
                    }
            return bytes;
        }
    } // namespace
    SHL_FUNC Ciphertext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return ct_load(thisptr, context, 0, true, inptr, size, in_bytes, true);
    }
    SHL_FUNC Ciphertext_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return ct_load(thisptr, context, 0, true, inptr, size, in_bytes, false);
    }
    SHL_FUNC Ciphertext_LoadItem(void *thisptr, void *context, uint64_t item, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return ct_load(thisptr, context, item, false, inptr, size, in_bytes, true);
    }
    SHL_FUNC Ciphertext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result)
    {
        return guarded({ thisptr, result }, [&] { save_size(compr_mode, result, [&] { return ct_raw_bytes(*as<Ciphertext>(thisptr)); }); });
    }
    SHL_FUNC Ciphertext_SaveItem(void *thisptr, uint64_t item, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes)
    {
        return guarded({ thisptr, outptr, out_bytes }, [&] {
            Ciphertext &ct = *as<Ciphertext>(thisptr);
            save_stream(outptr, size, compr_mode, out_bytes, [&] { return ct_raw_bytes(ct); }, [&](uint8_t *dst, size_t capacity) {
                if (item >= ct.batch())
                    throw std::out_of_range("batch item");
                const size_t poly_words = ct.coeff_modulus_size() * ct.poly_modulus_degree();
                size_t data_offset = 0;
                serial::save_ciphertext(ct.level() ? ct.level()->parms_id : kParmsIdZero, ct.is_ntt_form(), ct.size(), ct.poly_modulus_degree(),
                                        ct.coeff_modulus_size(), ct.scale(), ct.correction_factor(), nullptr, dst, capacity, &data_offset);
                // the coefficient words go from the device slab straight into the stream
                hip_ok(hipDeviceSynchronize(), "sync");
                for (size_t p = 0; p < ct.size(); p++)
                    hip_ok(hipMemcpy(dst + data_offset + p * poly_words * 8, ct.plane(p) + item * poly_words, poly_words * 8, hipMemcpyDeviceToHost), "D2H");
            });
        });
    }
    SHL_FUNC Ciphertext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes)
    {
        // (the batch is looked at before outptr and out_bytes are: a batch of two is refused whatever they are)
        const SHL_HRESULT refused = guarded({ thisptr }, [&] {
            if (as<Ciphertext>(thisptr)->batch() != 1)
                throw std::invalid_argument("Ciphertext_Save needs a batch of one: use Ciphertext_SaveItem for a slot of a batch");
        });
        return refused != SHL_S_OK ? refused : Ciphertext_SaveItem(thisptr, 0, outptr, size, compr_mode, out_bytes);
    }
    SHL_FUNC Plaintext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return pt_load(thisptr, context, inptr, size, in_bytes, true);
    }
    SHL_FUNC Plaintext_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return pt_load(thisptr, context, inptr, size, in_bytes, false);
    }
    SHL_FUNC Plaintext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result)
    {
        return guarded({ thisptr, result }, [&] {
            save_size(compr_mode, result, [&] { return serial::plaintext_save_size(as<Plaintext>(thisptr)->coeff_count()); });
        });
    }
    SHL_FUNC Plaintext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes)
    {
        return guarded({ thisptr, outptr, out_bytes }, [&] {
            Plaintext &pt = *as<Plaintext>(thisptr);
            save_stream(outptr, size, compr_mode, out_bytes, [&] { return serial::plaintext_save_size(pt.coeff_count()); },
                        [&](uint8_t *dst, size_t capacity) {
                            size_t data_offset = 0;
                            serial::save_plaintext(pt.level() ? pt.level()->parms_id : kParmsIdZero, pt.coeff_count(), pt.scale(), nullptr, dst,
                                                   capacity, &data_offset);
                            hip_ok(hipDeviceSynchronize(), "sync");
                            if (pt.coeff_count())
                                hip_ok(hipMemcpy(dst + data_offset, pt.data(), pt.coeff_count() * 8, hipMemcpyDeviceToHost), "D2H");
                        });
        });
    }
    SHL_FUNC KSwitchKeys_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result)
    {
        return guarded({ thisptr, result }, [&] { save_size(compr_mode, result, [&] { return ks_raw_size(*as<KSwitchKeys>(thisptr)); }); });
    }
    SHL_FUNC KSwitchKeys_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes)
    {
        return guarded({ thisptr, outptr, out_bytes }, [&] {
            KSwitchKeys &keys = *as<KSwitchKeys>(thisptr);
            save_stream(outptr, size, compr_mode, out_bytes, [&] { return ks_raw_size(keys); }, [&](uint8_t *dst, size_t capacity) {
                const size_t raw_bytes = ks_raw_size(keys);
                // A short uncompressed buffer is an invalid argument here, where the reference (serialization.cpp:36-54) and the
                // other five objects answer a buffer of at least a header with an I/O failure: tests/serial_cases.py:228 pins it
                if (capacity < raw_bytes)
                    throw std::invalid_argument("capacity");
                const Context *c = keys.context();
                serial::Writer w(dst, capacity, raw_bytes);
                w.header(raw_bytes);
                w.put(c ? c->key_level().parms_id : kParmsIdZero, 32);
                w.put64(keys.slots());
                for (size_t index = 0; index < keys.slots(); index++)
                {
                    const size_t digits = keys.has_key(index) ? keys.key(index).digits : 0;
                    w.put64(digits);
                    if (!digits)
                        continue;
                    const size_t n = c->n(), L = c->key_level().K, words = 2 * L * n;
                    Scratch natural(words); // one digit at a time: the transient device memory of a save is 2 L N words, not a whole key
                    for (size_t j = 0; j < digits; j++)
                    {
                        size_t off = 0;
                        const size_t bytes = serial::save_ciphertext(c->key_level().parms_id, true, 2, n, L, 1.0, 1, nullptr, dst + w.offset(),
                                                                     raw_bytes - w.offset(), &off);
                        keys.digit_words(index, j, natural.p);
                        hip_ok(hipMemcpy(dst + w.offset() + off, natural.p, words * 8, hipMemcpyDeviceToHost), "D2H");
                        w.skip(bytes);
                    }
                }
            });
        });
    }
    SHL_FUNC KSwitchKeys_DeviceBytes(void *thisptr, uint64_t *bytes)
    {
        return guarded({ thisptr, bytes }, [&] { *bytes = as<KSwitchKeys>(thisptr)->device_bytes(); });
    }
    SHL_FUNC KSwitchKeys_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return ks_load(thisptr, context, inptr, size, in_bytes, true);
    }
    SHL_FUNC KSwitchKeys_UnsafeLoad(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes)
    {
        return ks_load(thisptr, context, inptr, size, in_bytes, false);
    }

    // ------------------------------------------------------------------ Plaintext (native/src/seal/c/plaintext.h)
    SHL_FUNC Plaintext_Create1(void *context, void **plaintext)
    {
        return guarded({ context, plaintext }, [&] { *plaintext = new Plaintext(*as<Context>(context)); });
    }
    SHL_FUNC Plaintext_Create5(void *copy, void **plaintext)
    {
        return guarded({ copy, plaintext }, [&] { *plaintext = new Plaintext(*as<Plaintext>(copy)); });
    }
    SHL_FUNC Plaintext_Destroy(void *thisptr)
    {
        return guarded({ thisptr }, [&] { delete as<Plaintext>(thisptr); });
    }
    SHL_FUNC Plaintext_Set4(void *thisptr, uint64_t count, uint64_t *coeffs)
    {
        // (coeffs is looked at when there is something to read)
        return guarded({ thisptr, count ? coeffs : thisptr }, [&] { as<Plaintext>(thisptr)->set(coeffs, count, false); });
    }
    SHL_FUNC Plaintext_SetFromDevice(void *thisptr, uint64_t count, const uint64_t *device_coeffs)
    {
        return guarded({ thisptr, count ? device_coeffs : thisptr }, [&] { as<Plaintext>(thisptr)->set(device_coeffs, count, true); });
    }
    SHL_FUNC Plaintext_CoeffCount(void *thisptr, uint64_t *coeff_count)
    {
        return guarded({ thisptr, coeff_count }, [&] { *coeff_count = as<Plaintext>(thisptr)->coeff_count(); });
    }
    SHL_FUNC Plaintext_IsNTTForm(void *thisptr, bool *is_ntt_form)
    {
        return guarded({ thisptr, is_ntt_form }, [&] { *is_ntt_form = as<Plaintext>(thisptr)->is_ntt_form(); });
    }
    SHL_FUNC Plaintext_GetParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] { copy_parms_id(parms_id, as<Plaintext>(thisptr)->level()); });
    }
    SHL_FUNC Plaintext_SetParmsId(void *thisptr, uint64_t *parms_id)
    {
        return guarded({ thisptr, parms_id }, [&] {
            auto pt = as<Plaintext>(thisptr);
            const Level *l = std::memcmp(parms_id, kParmsIdZero, 32) ? pt->context().level_by_parms_id(parms_id) : nullptr;
            if (!l && std::memcmp(parms_id, kParmsIdZero, 32))
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            pt->set_level(l); // parms_id_zero: coefficient form
        });
    }
    SHL_FUNC Plaintext_Scale(void *thisptr, double *scale)
    {
        return guarded({ thisptr, scale }, [&] { *scale = as<Plaintext>(thisptr)->scale(); });
    }
    SHL_FUNC Plaintext_SetScale(void *thisptr, double scale)
    {
        return guarded({ thisptr }, [&] { as<Plaintext>(thisptr)->scale() = scale; });
    }
    SHL_FUNC Plaintext_CopyToHost(void *thisptr, uint64_t *dst, uint64_t word_count)
    {
        return guarded({ thisptr, dst }, [&] {
            auto pt = as<Plaintext>(thisptr);
            if (word_count != pt->coeff_count())
                throw std::invalid_argument("word_count does not match the plaintext");
            if (word_count)
            {
                if (hipDeviceSynchronize() != hipSuccess ||
                    (copy_d2h(dst, pt->data(), word_count * 8), false))
                    throw std::runtime_error("HIP failure in Plaintext_CopyToHost");
            }
        });
    }
}
