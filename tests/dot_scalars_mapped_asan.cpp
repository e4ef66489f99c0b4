// Stand-alone host-side check of the raw seam of the sparse scalar-weights product (include/sealhip.h: shl_dot_scalars_mapped) for
// a sanitizer: the library's sources built against the emulator in tests/hipemu with -fsanitize=address,undefined and linked with
// this main (seal_amd/csrc/Makefile: asan_dot_scalars_mapped).  Not a pytest test; it is run by hand on the CPU, never on a GPU.
// At N = 8 (lists and weights read per lane) and N = 128 (per wave) it runs ragged maps - one-term rows, an item and a weight named
// twice, the last item and the last weight, rows around the wide flush interval - in both weight forms, sizes 1 to 3, one launch,
// the library's cut and forced cuts, with the input, the weights, the result and the scratch in allocations of exactly their size:
// the emulated kernels run on the host, so a list entry, a weight or an operand read, or a result written, outside its allocation
// is the sanitizer's to report - the redzones of the allocator are the guard.  Every word is compared with the sum formed here
// in 128-bit host arithmetic; then every refusal of the seam.
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
static void refused(SHL_HRESULT hr, const char *what)
{
    if ((hr & 0xffffffffL) != (SHL_E_INVALIDARG & 0xffffffffL))
    {
        std::fprintf(stderr, "not refused: %s -> %lx\n", what, (unsigned long)hr);
        std::exit(1);
    }
    refusals++;
}

struct Device // an allocation of exactly `bytes` bytes
{
    void *p = nullptr;
    explicit Device(size_t bytes) { OK(shl_malloc(bytes ? bytes : 8, &p)); }
    ~Device() { shl_free(p); }
};

static uint64_t seed = 1;
static uint64_t next()
{
    return seed = seed * 6364136223846793005ull + 1442695040888963407ull;
}

static long run_ring(uint64_t n)
{
    int bits[3] = { 30, 30, 30 };
    uint64_t primes[3];
    OK(CoeffModulus_Create1(n, 3, bits, primes));
    void *parms = nullptr, *context = nullptr;
    OK(EncParams_Create1(2, &parms)); // CKKS
    OK(EncParams_SetPolyModulusDegree(parms, n));
    OK(EncParams_SetCoeffModulus(parms, 3, primes));
    OK(SEALContext_Create(parms, true, 0, &context));
    const uint64_t chain_index = 1, K = 2; // the first data level: the last prime is the special one
    const uint64_t words = K * n;
    long launches = 0;

    // row lengths of the maps; items and weights are drawn with repeats, the last of each is named by the last term
    const std::vector<std::vector<uint64_t>> maps = { { 1, 3, 7, 2 }, { 1, 4, 23, 9 }, { 255, 1, 256, 257, 3 } };
    for (const auto &lengths : maps)
    {
        const uint64_t items = 7, count = 5, rows = lengths.size();
        std::vector<uint64_t> off(1, 0), first, second;
        uint64_t longest = 0;
        for (uint64_t len : lengths)
        {
            for (uint64_t t = 0; t < len; t++)
            {
                first.push_back(t == 1 ? first.back() : (next() >> 33) % items); // an item named twice in a row
                second.push_back(t == 2 ? second.back() : (next() >> 33) % count);
            }
            off.push_back(first.size());
            longest = len > longest ? len : longest;
        }
        first.back() = items - 1;
        second.back() = count - 1;
        void *map = nullptr;
        OK(ItemMap_Create(context, rows, off.data(), first.data(), second.data(), items, count, &map));
        for (int narrow = 0; narrow < 2; narrow++)
        {
            // weights: wide [count][K] canonical words with q - 1 among them, narrow [count] signed 32-bit integers with the extremes
            std::vector<uint64_t> wide(count * K);
            std::vector<int32_t> ints(count);
            for (size_t i = 0; i < count; i++)
            {
                ints[i] = i == 0 ? INT32_MIN : i == 1 ? INT32_MAX : (int32_t)(next() >> 32);
                for (uint64_t k = 0; k < K; k++)
                    wide[i * K + k] = i % 2 == 0 ? primes[k] - 1 : next() % primes[k];
            }
            Device w(narrow ? count * 4 : wide.size() * 8); // (narrow: 20 bytes - the allocator aligns it to 16, as the call requires)
            if (narrow)
                OK(shl_memcpy_h2d(w.p, ints.data(), count * 4));
            else
                OK(shl_memcpy_h2d(w.p, wide.data(), wide.size() * 8));
            for (uint64_t size = 1; size <= 3; size++)
            {
                std::vector<uint64_t> x(size * items * words), want(size * rows * words), got(want.size());
                for (size_t i = 0; i < x.size(); i++)
                    x[i] = i % 3 != 2 ? primes[i / n % K] - 1 : next() % primes[i / n % K];
                for (uint64_t p = 0; p < size; p++)
                    for (uint64_t o = 0; o < rows; o++)
                        for (uint64_t k = 0; k < K; k++)
                            for (uint64_t j = 0; j < n; j++)
                            {
                                const uint64_t q = primes[k];
                                uint64_t sum = 0;
                                for (uint64_t t = off[o]; t < off[o + 1]; t++)
                                {
                                    const uint64_t wk = narrow ? (uint64_t)(((int64_t)ints[second[t]] % (int64_t)q + (int64_t)q) % (int64_t)q)
                                                               : wide[second[t] * K + k];
                                    const uint64_t a = x[((p * items + first[t]) * K + k) * n + j];
                                    sum = (uint64_t)((sum + (unsigned __int128)a * wk) % q);
                                }
                                want[((p * rows + o) * K + k) * n + j] = sum;
                            }
                Device a(x.size() * 8), r(got.size() * 8);
                OK(shl_memcpy_h2d(a.p, x.data(), x.size() * 8));
                for (uint64_t slices : { uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(23) })
                {
                    if (slices > longest)
                        continue;
                    uint64_t used = 0;
                    OK(shl_dot_scalars_mapped(context, chain_index, w.p, count, narrow, (const uint64_t *)a.p, items, nullptr, size, map, slices, nullptr,
                                              &used, nullptr));
                    if (!used)
                        return -1;
                    Device scratch(used > 1 ? used * got.size() * 8 : 0);
                    OK(shl_dot_scalars_mapped(context, chain_index, w.p, count, narrow, (const uint64_t *)a.p, items, (uint64_t *)r.p, size, map, slices,
                                              used > 1 ? (uint64_t *)scratch.p : nullptr, &used, nullptr));
                    OK(shl_device_synchronize());
                    OK(shl_memcpy_d2h(got.data(), r.p, got.size() * 8));
                    if (got != want)
                    {
                        std::fprintf(stderr, "wrong words: N %lu, longest row %lu, narrow %d, size %lu, slices %lu (%lu run)\n", (unsigned long)n,
                                     (unsigned long)longest, narrow, (unsigned long)size, (unsigned long)slices, (unsigned long)used);
                        std::exit(1);
                    }
                    launches++;
                }
            }
            // the seam's refusals, as queries and once with operands
            uint64_t used = 0;
            const auto query = [&](uint64_t sz, uint64_t a_batch, uint64_t weights, uint64_t slices, uint64_t ci = 1) {
                return shl_dot_scalars_mapped(context, ci, nullptr, weights, narrow, nullptr, a_batch, nullptr, sz, map, slices, nullptr, &used, nullptr);
            };
            OK(query(2, items, count, 0));
            refused(query(0, items, count, 0), "size 0");
            refused(query(17, items, count, 0), "size 17");
            refused(query(2, items - 1, count, 0), "a batch that is not the map's");
            refused(query(2, items, count + 1, 0), "a weight count that is not the map's");
            refused(query(2, items, count, longest + 1), "more slices than the longest row has terms");
            refused(query(2, items, count, 65), "more than 64 slices");
            if ((query(2, items, count, 0, 99) & 0xffffffffL) == 0)
                return -1; // an unknown level
            if (longest >= 2)
            {
                Device a(2 * items * words * 8), r(2 * rows * words * 8);
                refused(shl_dot_scalars_mapped(context, chain_index, w.p, count, narrow, (const uint64_t *)a.p, items, (uint64_t *)r.p, 2, map, 2, nullptr,
                                               &used, nullptr),
                        "a cut without scratch");
            }
        }
        OK(ItemMap_Destroy(map));
    }
    SEALContext_Destroy(context);
    EncParams_Destroy(parms);
    return launches;
}

int main()
{
    long launches = 0;
    for (uint64_t n : { uint64_t(8), uint64_t(128) })
    {
        const long l = run_ring(n);
        if (l < 0)
            return 1;
        launches += l;
    }
    uint64_t flush = 0, narrow_flush = 0;
    OK(shl_dot_scalars_mapped_info(&flush, &narrow_flush));
    if (flush != 256 || narrow_flush != 1024)
        return 1;
    std::printf("dot_scalars_mapped_asan: %ld launches word for word, %d refusals, no report\n", launches, refusals);
    return 0;
}
