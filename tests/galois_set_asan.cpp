// Stand-alone host-side check of Galois sets (include/sealhip.h: GaloisSet_Create, Evaluator_ApplyGaloisSet) for a sanitizer: the
// library's sources built against the emulator in tests/hipemu with -fsanitize=address,undefined and linked with this main
// (seal_amd/csrc/Makefile: asan_galois_set).  Not a pytest test; it is run by hand on the CPU, never on a GPU.
// It walks set creation and every refusal of the two constructors and of the call, then makes set calls - a set from steps with
// identity entries and a repeat, a set from elements with the conjugation - at N = 8, 64 and 1024 (the loop over the entries) and at
// N = 8192 on both sub-routes of the one-batch route (SEALHIP_KS_SPLIT = 1: the operand read through the entries' maps; 3: permuted
// scratch), chunked once, in all three schemes, with operands, keys and results in allocations of exactly their size: the emulated
// kernels run on the host, so a table row, a key or an operand read, or a result written, outside its allocation is the sanitizer's to
// report.  Every result item is compared word for word with the single-key call on a batch of one.
#include "../include/sealhip.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static int refusals = 0;
static void refused(SHL_HRESULT hr, const char *what, SHL_HRESULT want = SHL_E_INVALIDARG)
{
    if ((hr & 0xffffffffL) != (want & 0xffffffffL))
    {
        std::fprintf(stderr, "not refused: %s -> %lx\n", what, (unsigned long)hr);
        std::exit(1);
    }
    refusals++;
}

static uint64_t seed = 1;
static uint64_t next()
{
    return seed = seed * 6364136223846793005ull + 1442695040888963407ull;
}

struct Ring
{
    int scheme; // 1 BFV, 2 CKKS, 3 BGV
    uint64_t n, L;
    std::vector<uint64_t> primes;
    void *parms = nullptr, *context = nullptr, *ev = nullptr, *keys = nullptr;
    uint64_t first[4];
    uint64_t correction = 1;
    Ring(int scheme_, uint64_t n_, std::vector<int> bits) : scheme(scheme_), n(n_), L(bits.size()), primes(bits.size())
    {
        if (scheme == 3)
            correction = 3;
        OK(CoeffModulus_Create1(n, L, bits.data(), primes.data()));
        OK(EncParams_Create1((uint8_t)scheme, &parms));
        OK(EncParams_SetPolyModulusDegree(parms, n));
        OK(EncParams_SetCoeffModulus(parms, L, primes.data()));
        if (scheme != 2)
        {
            uint64_t t = 0;
            OK(PlainModulus_Batching(n, 20, &t));
            OK(EncParams_SetPlainModulus2(parms, t));
        }
        OK(SEALContext_Create(parms, true, 0, &context));
        OK(SEALContext_FirstParmsId(context, first));
        OK(Evaluator_Create(context, &ev));
        OK(KSwitchKeys_Create1(&keys));
    }
    ~Ring()
    {
        KSwitchKeys_Destroy(keys);
        Evaluator_Destroy(ev);
        SEALContext_Destroy(context);
        EncParams_Destroy(parms);
    }
    uint64_t K() const { return L - 1; }
    uint32_t elt(int step) const
    {
        uint32_t e = 0;
        OK(GaloisTool_GetEltFromStep(context, step, &e));
        return e;
    }
    void add_key(uint32_t e) // uniform words, the ends of the range among them
    {
        std::vector<uint64_t> w(K() * 2 * L * n);
        for (size_t i = 0; i < w.size(); i++)
        {
            const uint64_t q = primes[i / n % L];
            w[i] = i % 5 == 0 ? q - 1 : i % 7 == 0 ? 0 : next() % q;
        }
        OK(KSwitchKeys_SetKey(keys, context, (e - 1) >> 1, K(), w.data()));
    }
    void *ciphertext(const std::vector<uint64_t> &words, uint64_t batch) // [2][batch][K][N]
    {
        void *c = nullptr;
        OK(Ciphertext_CreateBatch(context, batch, &c));
        OK(Ciphertext_Resize1(c, context, first, 2));
        OK(Ciphertext_SetIsNTTForm(c, scheme != 1));
        OK(Ciphertext_SetScale(c, scheme == 2 ? 1048576.0 : 1.0));
        OK(Ciphertext_SetCorrectionFactor(c, correction));
        OK(Ciphertext_CopyFromHost(c, words.data(), words.size()));
        return c;
    }
    std::vector<uint64_t> operand(uint64_t batch)
    {
        std::vector<uint64_t> x(2 * batch * K() * n);
        for (size_t i = 0; i < x.size(); i++)
        {
            const uint64_t q = primes[i / n % K()];
            x[i] = i % 3 == 0 ? q - 1 : i % 11 == 0 ? q / 2 : next() % q;
        }
        return x;
    }
};

// one set call against the single-key calls -> result items compared
static long check_call(Ring &r, void *set, const std::vector<uint32_t> &elts, uint64_t B)
{
    const uint64_t R = elts.size(), KN = r.K() * r.n;
    const std::vector<uint64_t> x = r.operand(B);
    void *c = r.ciphertext(x, B), *dest = nullptr;
    OK(Ciphertext_CreateBatch(r.context, B * R, &dest));
    OK(Evaluator_ApplyGaloisSet(r.ev, c, set, dest));
    std::vector<uint64_t> got(2 * B * R * KN);
    OK(Ciphertext_CopyToHost(dest, got.data(), got.size()));
    long items = 0;
    for (uint64_t b = 0; b < B; b++)
        for (uint64_t e = 0; e < R; e++)
        {
            std::vector<uint64_t> one(2 * KN), want(2 * KN);
            for (uint64_t p = 0; p < 2; p++)
                for (uint64_t w = 0; w < KN; w++)
                    one[p * KN + w] = x[(p * B + b) * KN + w];
            if (elts[e])
            {
                void *c1 = r.ciphertext(one, 1), *d1 = nullptr;
                OK(Ciphertext_CreateBatch(r.context, 1, &d1));
                OK(Evaluator_ApplyGalois(r.ev, c1, elts[e], r.keys, d1, nullptr));
                OK(Ciphertext_CopyToHost(d1, want.data(), want.size()));
                Ciphertext_Destroy(d1);
                Ciphertext_Destroy(c1);
            }
            else
                want = one; // an identity entry: a copy
            for (uint64_t p = 0; p < 2; p++)
                for (uint64_t w = 0; w < KN; w++)
                    if (got[(p * B * R + b * R + e) * KN + w] != want[p * KN + w])
                    {
                        std::fprintf(stderr, "wrong words: scheme %d, N %lu, item %lu, entry %lu, polynomial %lu, word %lu\n", r.scheme,
                                     (unsigned long)r.n, (unsigned long)b, (unsigned long)e, (unsigned long)p, (unsigned long)w);
                        std::exit(1);
                    }
            items++;
        }
    Ciphertext_Destroy(dest);
    Ciphertext_Destroy(c);
    return items;
}

static long run_ring(int scheme, uint64_t n, const std::vector<int> &bits, bool sub_routes)
{
    Ring r(scheme, n, bits);
    const int far = -(int)(n / 2 - 1);
    const uint32_t e1 = r.elt(1), efar = r.elt(far), conj = (uint32_t)(2 * n - 1);
    r.add_key(e1);
    r.add_key(efar);
    r.add_key(conj);
    long items = 0;
    // creation and its refusals
    void *set = nullptr, *from_steps = nullptr, *probe = nullptr;
    const std::vector<uint32_t> elts = { e1, conj, efar, e1, conj };
    const std::vector<int> steps = { 1, 0, far, 1, 0 };
    const std::vector<uint32_t> steps_as_elts = { e1, 0, efar, e1, 0 };
    OK(GaloisSet_Create(r.context, r.keys, elts.size(), elts.data(), &set));
    OK(GaloisSet_CreateFromSteps(r.context, r.keys, steps.size(), steps.data(), &from_steps));
    uint64_t count = 0, identities = 0, distinct = 0;
    bool register_order = false;
    OK(GaloisSet_Info(from_steps, &count, &identities, &distinct, &register_order));
    OK(GaloisSet_Info(from_steps, nullptr, nullptr, nullptr, nullptr));
    if (count != 5 || identities != 2 || distinct != (e1 == efar ? 1u : 2u) || register_order != (n >= 8192)) // (step -(N/2 - 1) is step +1 again)
        return -1;
    const uint32_t even[2] = { e1, 2 }, large[1] = { (uint32_t)(2 * n + 1) }, absent[1] = { r.elt(2) }, zero[1] = { 0 };
    const int absent_step[1] = { 2 }, large_step[1] = { (int)n };
    refused(GaloisSet_Create(r.context, r.keys, 2, even, &probe), "an even element");
    refused(GaloisSet_Create(r.context, r.keys, 1, zero, &probe), "element 0");
    refused(GaloisSet_Create(r.context, r.keys, 1, large, &probe), "an element >= 2N");
    refused(GaloisSet_Create(r.context, r.keys, 1, absent, &probe), "a missing key");
    refused(GaloisSet_CreateFromSteps(r.context, r.keys, 1, absent_step, &probe), "a step whose key is missing");
    refused(GaloisSet_CreateFromSteps(r.context, r.keys, 1, large_step, &probe), "a step too large");
    refused(GaloisSet_Create(r.context, r.keys, 0, elts.data(), &probe), "count 0");
    refused(GaloisSet_CreateFromSteps(r.context, r.keys, 0, steps.data(), &probe), "count 0");
    refused(GaloisSet_Create(r.context, r.keys, 1, nullptr, &probe), "a NULL array");
    refused(GaloisSet_CreateFromSteps(r.context, r.keys, 1, nullptr, &probe), "a NULL array");
    refused(GaloisSet_Create(nullptr, r.keys, 1, elts.data(), &probe), "a NULL context", SHL_E_POINTER);
    refused(GaloisSet_Create(r.context, nullptr, 1, elts.data(), &probe), "NULL keys", SHL_E_POINTER);
    refused(GaloisSet_Create(r.context, r.keys, 1, elts.data(), nullptr), "a NULL output", SHL_E_POINTER);
    refused(GaloisSet_Destroy(nullptr), "destroying NULL", SHL_E_POINTER);
    {
        Ring other(scheme, n, bits);
        other.add_key(e1);
        refused(GaloisSet_Create(r.context, other.keys, 1, elts.data(), &probe), "keys of another context");
    }
    // the call's refusals
    {
        const std::vector<uint64_t> x = r.operand(2);
        void *c = r.ciphertext(x, 2), *wrong = nullptr, *right = nullptr;
        OK(Ciphertext_CreateBatch(r.context, 9, &wrong));
        OK(Ciphertext_CreateBatch(r.context, 10, &right));
        refused(Evaluator_ApplyGaloisSet(r.ev, c, set, c), "destination == encrypted");
        refused(Evaluator_ApplyGaloisSet(r.ev, c, set, wrong), "a destination of another batch");
        refused(Evaluator_ApplyGaloisSet(r.ev, c, nullptr, right), "a NULL set", SHL_E_POINTER);
        r.add_key(conj); // a key replaced after Create
        refused(Evaluator_ApplyGaloisSet(r.ev, c, set, right), "a replaced key");
        OK(Evaluator_ApplyGaloisSet(r.ev, c, from_steps, right)); // (that set does not name the replaced key)
        OK(GaloisSet_Destroy(set));
        OK(GaloisSet_Create(r.context, r.keys, elts.size(), elts.data(), &set));
        Ciphertext_Destroy(right);
        Ciphertext_Destroy(wrong);
        Ciphertext_Destroy(c);
    }
    // set calls, word for word
    const char *splits[] = { nullptr, "1", "3" };
    for (int s = 0; s < (sub_routes ? 3 : 1); s++)
    {
        if (splits[s])
            setenv("SEALHIP_KS_SPLIT", splits[s], 1);
        for (uint64_t B : { uint64_t(1), uint64_t(3) })
        {
            if (sub_routes && B == 3 && s == 0)
                continue; // (the rule's own choice at this size is the digit groups: covered by "3")
            items += check_call(r, set, elts, B);
            items += check_call(r, from_steps, steps_as_elts, B);
        }
        unsetenv("SEALHIP_KS_SPLIT");
    }
    if (sub_routes && scheme == 2)
    {
        // 15 virtual items in chunks of 2 on 3 lanes: edges inside a run of one key and between keys, the last chunk short
        setenv("SEALHIP_KS_SPLIT", "1", 1);
        setenv("SEALHIP_KS_CHUNK", "2", 1);
        setenv("SEALHIP_KS_LANES", "3", 1);
        items += check_call(r, set, elts, 3);
        unsetenv("SEALHIP_KS_SPLIT");
        unsetenv("SEALHIP_KS_CHUNK");
        unsetenv("SEALHIP_KS_LANES");
    }
    // destroying the set right after a call
    {
        const std::vector<uint64_t> x = r.operand(1);
        void *c = r.ciphertext(x, 1), *dest = nullptr;
        OK(Ciphertext_CreateBatch(r.context, 5, &dest));
        OK(Evaluator_ApplyGaloisSet(r.ev, c, set, dest));
        OK(GaloisSet_Destroy(set));
        OK(GaloisSet_Destroy(from_steps));
        OK(Evaluator_Synchronize(r.ev));
        Ciphertext_Destroy(dest);
        Ciphertext_Destroy(c);
    }
    return items;
}

int main()
{
    long items = 0;
    for (int scheme : { 2, 1, 3 })
    {
        const long small[] = { run_ring(scheme, 8, { 30, 30, 30 }, false), run_ring(scheme, 64, { 60, 40, 40, 60 }, false),
                               run_ring(scheme, 1024, { 60, 40, 60 }, false), run_ring(scheme, 8192, { 60, 40, 40, 60 }, true) };
        for (long l : small)
        {
            if (l < 0)
                return 1;
            items += l;
        }
    }
    uint64_t batched = 0, looped = 0, fused = 0;
    OK(SealHip_GaloisSetStats(&batched, &looped, &fused));
    if (!batched || !looped || fused < batched)
        return 1;
    std::printf("galois_set_asan: %ld result items word for word (%lu calls on the one-batch route, %lu on the loop), %d refusals, no report\n", items,
                (unsigned long)batched, (unsigned long)looped, refusals);
    return 0;
}
