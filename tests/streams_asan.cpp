// Stand-alone host-side check of the object streams (include/sealhip.h: *_SaveSize, *_Save, *_Load of Ciphertext, Plaintext,
// KSwitchKeys, SecretKey, PublicKey and EncryptionParameters) for a sanitizer: the library's sources built against the emulator in
// tests/hipemu with -fsanitize=address,undefined and linked with this main (seal_amd/csrc/Makefile: asan_streams).  Not a pytest
// test; it is run by hand on the CPU, never on a GPU.  At CKKS N = 64 {40, 30, 30, 40} every object is saved into a heap buffer of
// exactly the capacity given - 8, 16, 64, cap - 1 and cap bytes, cap = *_SaveSize(none) - in every compression mode (none, zlib,
// zstd when the library finds it, an unknown one): the save path is pointer arithmetic on the caller's buffer, and the redzones of
// the allocator catch a byte written past it.  A save that succeeds wrote no more than the capacity; the stream written at
// capacity cap is loaded into an empty object, whose own stream has to equal the original's.
#include "../include/sealhip.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define OK(call)                                                                \
    do                                                                          \
    {                                                                           \
        const SHL_HRESULT hr_ = (call);                                         \
        if (hr_ != SHL_S_OK)                                                    \
        {                                                                       \
            std::fprintf(stderr, "%s:%d: %s -> %lx\n", __FILE__, __LINE__, #call, (unsigned long)hr_); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

// the emulator keeps its fiber stacks (tests/hipemu/hip_emu.cpp) to the end of the process: not what this program is about
extern "C" const char *__asan_default_options()
{
    return "detect_leaks=0";
}

typedef SHL_HRESULT (*SaveSize)(void *, uint8_t, int64_t *);
typedef SHL_HRESULT (*Save)(void *, uint8_t *, uint64_t, uint8_t, int64_t *);
typedef SHL_HRESULT (*Load)(void *, void *, uint8_t *, uint64_t, int64_t *);

struct Kind
{
    const char *name;
    void *object, *empty; // `empty` takes the streams loaded back
    SaveSize save_size;
    Save save;
    Load load; // null: EncParams_Load, which takes no context
};

// the stream written into an allocation of exactly `capacity` bytes; empty when the save is refused
static std::vector<uint8_t> save_exact(const Kind &k, void *object, size_t capacity, uint8_t mode, SHL_HRESULT *hr)
{
    std::unique_ptr<uint8_t[]> buffer(new uint8_t[capacity]);
    int64_t written = -1;
    *hr = k.save(object, buffer.get(), capacity, mode, &written);
    if (*hr != SHL_S_OK)
        return {};
    if (written < 16 || (size_t)written > capacity)
    {
        std::fprintf(stderr, "%s: %lld bytes reported for a capacity of %zu\n", k.name, (long long)written, capacity);
        std::exit(1);
    }
    return std::vector<uint8_t>(buffer.get(), buffer.get() + written);
}

static std::vector<uint8_t> whole_stream(const Kind &k, void *object)
{
    int64_t cap = 0;
    OK(k.save_size(object, 0, &cap));
    SHL_HRESULT hr;
    std::vector<uint8_t> s = save_exact(k, object, (size_t)cap, 0, &hr);
    OK(hr);
    return s;
}

int main()
{
    const uint64_t n = 64;
    int bits[4] = { 40, 30, 30, 40 };
    uint64_t primes[4], seed[8] = { 1, 2, 3, 4, 5, 6, 7, 8 }, first[4];
    OK(CoeffModulus_Create1(n, 4, bits, primes));
    void *parms = nullptr, *parms2 = nullptr, *context = nullptr, *kg = nullptr, *encryptor = nullptr;
    OK(EncParams_Create1(2, &parms)); // CKKS
    OK(EncParams_Create1(2, &parms2));
    OK(EncParams_SetPolyModulusDegree(parms, n));
    OK(EncParams_SetCoeffModulus(parms, 4, primes));
    OK(SEALContext_Create(parms, true, 0, &context));
    OK(SEALContext_FirstParmsId(context, first));
    OK(KeyGenerator_Create1(context, seed, &kg));

    void *sk = nullptr, *sk2 = nullptr, *pk = nullptr, *pk2 = nullptr, *ksk = nullptr, *ksk2 = nullptr;
    void *ct = nullptr, *ct2 = nullptr, *pt = nullptr, *pt2 = nullptr;
    OK(SecretKey_Create(context, &sk));
    OK(SecretKey_Create(context, &sk2));
    OK(KeyGenerator_SecretKey(kg, sk));
    OK(PublicKey_Create(context, &pk));
    OK(PublicKey_Create(context, &pk2));
    OK(KeyGenerator_CreatePublicKey(kg, pk));
    OK(KSwitchKeys_Create1(&ksk));
    OK(KSwitchKeys_Create1(&ksk2));
    OK(KeyGenerator_CreateRelinKeys(kg, ksk));
    OK(Encryptor_Create(context, nullptr, sk, &encryptor));
    OK(Ciphertext_Create3(context, nullptr, &ct));
    OK(Ciphertext_Create3(context, nullptr, &ct2));
    OK(Encryptor_EncryptZeroSymmetric2(encryptor, false, ct, nullptr));
    std::vector<uint64_t> words(3 * n);
    for (size_t i = 0; i < words.size(); i++)
        words[i] = (i * 2654435761ull) % primes[i / n]; // an NTT-form plaintext of the first data level: every residue reduced
    OK(Plaintext_Create1(context, &pt));
    OK(Plaintext_Create1(context, &pt2));
    OK(Plaintext_Set4(pt, words.size(), words.data()));
    OK(Plaintext_SetParmsId(pt, first));
    OK(Plaintext_SetScale(pt, 1048576.0));

    const Kind kinds[6] = {
        { "Ciphertext", ct, ct2, Ciphertext_SaveSize, Ciphertext_Save, Ciphertext_Load },
        { "Plaintext", pt, pt2, Plaintext_SaveSize, Plaintext_Save, Plaintext_Load },
        { "KSwitchKeys", ksk, ksk2, KSwitchKeys_SaveSize, KSwitchKeys_Save, KSwitchKeys_Load },
        { "SecretKey", sk, sk2, SecretKey_SaveSize, SecretKey_Save, SecretKey_Load },
        { "PublicKey", pk, pk2, PublicKey_SaveSize, PublicKey_Save, PublicKey_Load },
        { "EncParams", parms, parms2, EncParams_SaveSize, EncParams_Save, nullptr },
    };
    long saves = 0, refused = 0, loads = 0;
    for (const Kind &k : kinds)
    {
        const std::vector<uint8_t> plain = whole_stream(k, k.object);
        const size_t cap = plain.size();
        for (uint8_t mode : { 0, 1, 2, 9 })
        {
            int64_t bound = 0;
            const bool known = k.save_size(k.object, mode, &bound) == SHL_S_OK; // zstd is looked up at run time
            if (!known && mode != 2 && mode != 9)
            {
                std::fprintf(stderr, "%s: mode %d refused\n", k.name, mode);
                return 1;
            }
            for (size_t capacity : { (size_t)8, (size_t)16, (size_t)64, cap - 1, cap })
            {
                SHL_HRESULT hr;
                std::vector<uint8_t> s = save_exact(k, k.object, capacity, mode, &hr);
                saves++;
                if (hr != SHL_S_OK)
                {
                    refused++;
                    if (known && mode == 0 && capacity == cap)
                    {
                        std::fprintf(stderr, "%s: the capacity its SaveSize names is refused (%lx)\n", k.name, (unsigned long)hr);
                        return 1;
                    }
                    continue;
                }
                if (!known || (mode == 0 && capacity < cap))
                {
                    std::fprintf(stderr, "%s: mode %d, capacity %zu of %zu accepted\n", k.name, mode, capacity, cap);
                    return 1;
                }
                if (capacity != cap)
                    continue;
                // the stream loads back (from an allocation of exactly its size) into an equal object
                std::unique_ptr<uint8_t[]> in(new uint8_t[s.size()]);
                std::memcpy(in.get(), s.data(), s.size());
                int64_t read = -1;
                if (k.load)
                    OK(k.load(k.empty, context, in.get(), s.size(), &read));
                else
                    OK(EncParams_Load(k.empty, in.get(), s.size(), &read));
                if ((size_t)read != s.size() || whole_stream(k, k.empty) != plain)
                {
                    std::fprintf(stderr, "%s: mode %d does not load back\n", k.name, mode);
                    return 1;
                }
                loads++;
            }
        }
    }
    OK(Encryptor_Destroy(encryptor));
    OK(KeyGenerator_Destroy(kg));
    for (void *p : { ct, ct2 })
        OK(Ciphertext_Destroy(p));
    for (void *p : { pt, pt2 })
        OK(Plaintext_Destroy(p));
    for (void *p : { ksk, ksk2 })
        OK(KSwitchKeys_Destroy(p));
    for (void *p : { sk, sk2 })
        OK(SecretKey_Destroy(p));
    for (void *p : { pk, pk2 })
        OK(PublicKey_Destroy(p));
    OK(SEALContext_Destroy(context));
    for (void *p : { parms, parms2 })
        OK(EncParams_Destroy(p));
    std::printf("streams_asan ok: %ld saves into exact allocations (%ld refused), %ld streams loaded back\n", saves, refused, loads);
    return 0;
}
