// Stand-alone host-side check of the convolution's raw seam (include/sealhip.h: shl_conv2d_scalars_tile) for a sanitizer: the
// library's sources built against the emulator in tests/hipemu with -fsanitize=address,undefined and linked with this main
// (seal_amd/csrc/Makefile: asan_conv2d).  Not a pytest test; it is run by hand on the CPU, never on a GPU.
// At N = 8 it runs the shape list of tests/conv2d_scalars_cases.py with the output channels taken in turn from the row counts of
// both tiles, both weight forms, the four layouts, both hints and the library's, one launch and forced cuts, with the input, the
// weights and the result in allocations of exactly their size - the emulated kernels run on the host, so a tap read or a result
// written outside the batch is the sanitizer's to report - and compares every word with the sum formed here; then every refusal.
#include "../include/sealhip.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Device // an allocation of exactly `words` words
{
    void *p = nullptr;
    explicit Device(size_t words) { OK(shl_malloc(words ? words * 8 : 8, &p)); }
    ~Device() { shl_free(p); }
};

int main()
{
    const uint64_t n = 8, size = 2;
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

    // (C, H, W, kh, kw, sh, sw, ph, pw)
    const uint64_t geometries[][9] = { { 2, 3, 4, 3, 3, 1, 1, 1, 1 }, { 3, 4, 5, 2, 3, 2, 1, 1, 2 }, { 2, 5, 5, 1, 1, 2, 2, 0, 0 }, { 3, 2, 3, 1, 1, 1, 1, 0, 0 },
                                       { 2, 3, 2, 3, 2, 1, 1, 0, 0 }, { 1, 1, 4, 1, 3, 1, 1, 0, 1 }, { 2, 5, 5, 2, 3, 2, 3, 1, 1 } };
    const uint64_t channels[] = { 1, 3, 4, 5, 9, 7, 8, 17 }; // the row counts of the tiles of 4 and 8
    uint64_t seed = 1;
    const auto next = [&]() { return seed = seed * 6364136223846793005ull + 1442695040888963407ull; };
    long launches = 0;
    unsigned turn = 0;
    for (const auto &g : geometries)
        for (unsigned rep = 0; rep < 2; rep++, turn++)
        {
            const SHL_CONV2D s{ g[0], g[1], g[2], channels[turn % 8], g[3], g[4], g[5], g[6], g[7], g[8] };
            const uint64_t oh = (s.height + 2 * s.pad_h - s.kernel_h) / s.stride_h + 1, ow = (s.width + 2 * s.pad_w - s.kernel_w) / s.stride_w + 1;
            const uint64_t inner = s.in_channels * s.kernel_h * s.kernel_w, in_items = s.in_channels * s.height * s.width,
                           out_items = s.out_channels * oh * ow;
            for (int narrow = 0; narrow < 2; narrow++)
            {
                // weights: wide [OC inner][K] canonical words, narrow [OC inner] signed 32-bit integers with the extremes among them
                std::vector<uint64_t> wide(s.out_channels * inner * K);
                std::vector<int32_t> ints(s.out_channels * inner + 1);
                for (size_t i = 0; i < s.out_channels * inner; i++)
                {
                    ints[i] = i == 0 ? INT32_MIN : i == 1 ? INT32_MAX : (int32_t)(next() >> 32);
                    for (uint64_t k = 0; k < K; k++)
                        wide[i * K + k] = i % 5 == 0 ? primes[k] - 1 : next() % primes[k];
                }
                Device w(narrow ? (s.out_channels * inner + 1) / 2 : wide.size());
                if (narrow)
                    OK(shl_memcpy_h2d(w.p, ints.data(), s.out_channels * inner * 4));
                else
                    OK(shl_memcpy_h2d(w.p, wide.data(), wide.size() * 8));
                for (uint64_t flags = 0; flags < 4; flags++)
                {
                    std::vector<uint64_t> x(size * in_items * words), want(size * out_items * words), got(want.size());
                    for (size_t i = 0; i < x.size(); i++)
                        x[i] = i % 7 == 0 ? primes[i / n % K] - 1 : next() % primes[i / n % K];
                    const auto in_at = [&](uint64_t c, uint64_t y, uint64_t xx) {
                        return flags & 1 ? (y * s.width + xx) * s.in_channels + c : (c * s.height + y) * s.width + xx;
                    };
                    const auto out_at = [&](uint64_t o, uint64_t y, uint64_t xx) { return flags & 2 ? (y * ow + xx) * s.out_channels + o : (o * oh + y) * ow + xx; };
                    for (uint64_t p = 0; p < size; p++)
                        for (uint64_t o = 0; o < s.out_channels; o++)
                            for (uint64_t y = 0; y < oh; y++)
                                for (uint64_t xx = 0; xx < ow; xx++)
                                    for (uint64_t k = 0; k < K; k++)
                                        for (uint64_t j = 0; j < n; j++)
                                        {
                                            const uint64_t q = primes[k];
                                            uint64_t sum = 0;
                                            for (uint64_t c = 0; c < s.in_channels; c++)
                                                for (uint64_t dy = 0; dy < s.kernel_h; dy++)
                                                    for (uint64_t dx = 0; dx < s.kernel_w; dx++)
                                                    {
                                                        const int64_t iy = (int64_t)(y * s.stride_h + dy) - (int64_t)s.pad_h,
                                                                      ix = (int64_t)(xx * s.stride_w + dx) - (int64_t)s.pad_w;
                                                        if (iy < 0 || ix < 0 || iy >= (int64_t)s.height || ix >= (int64_t)s.width)
                                                            continue;
                                                        const size_t t = o * inner + (c * s.kernel_h + dy) * s.kernel_w + dx;
                                                        const uint64_t wk = narrow ? (uint64_t)(((int64_t)ints[t] % (int64_t)q + (int64_t)q) % (int64_t)q) : wide[t * K + k];
                                                        const uint64_t a = x[((p * in_items + in_at(c, (uint64_t)iy, (uint64_t)ix)) * K + k) * n + j];
                                                        sum = (uint64_t)((sum + (unsigned __int128)a * wk) % q);
                                                    }
                                            want[((p * out_items + out_at(o, y, xx)) * K + k) * n + j] = sum;
                                        }
                    Device a(x.size()), r(got.size());
                    OK(shl_memcpy_h2d(a.p, x.data(), x.size() * 8));
                    for (uint64_t hint = 0; hint < 3; hint++)
                        for (uint64_t slices = 0; slices <= 3 && slices <= inner; slices++)
                            for (uint64_t tile : { uint64_t(0), uint64_t(4), uint64_t(8) })
                            {
                                if ((hint + slices + tile / 4 + flags) % 2 && tile) // every tile meets every hint, cut and layout over the list
                                    continue;
                                uint64_t used = 0;
                                OK(shl_conv2d_scalars_tile(context, chain_index, w.p, (const uint64_t *)a.p, (uint64_t *)r.p, size, &s, flags | (narrow ? 4 : 0),
                                                           slices, &used, tile, hint, nullptr));
                                OK(shl_device_synchronize());
                                OK(shl_memcpy_d2h(got.data(), r.p, got.size() * 8));
                                if (got != want || !used)
                                {
                                    std::fprintf(stderr, "wrong words: geometry %u, OC %lu, narrow %d, flags %lu, hint %lu, slices %lu, tile %lu\n", turn / 2,
                                                 (unsigned long)s.out_channels, narrow, (unsigned long)flags, (unsigned long)hint, (unsigned long)slices,
                                                 (unsigned long)tile);
                                    return 1;
                                }
                                launches++;
                            }
                    uint64_t used = 0;
                    OK(shl_conv2d_scalars(context, chain_index, w.p, (const uint64_t *)a.p, (uint64_t *)r.p, size, &s, flags | (narrow ? 4 : 0), 0, &used));
                    OK(shl_memcpy_d2h(got.data(), r.p, got.size() * 8));
                    if (got != want)
                        return 1;
                    launches++;
                }
            }
        }

    // every refusal, asked as a query (no result: nothing is allocated or launched) and, once each way, with operands
    const SHL_CONV2D good{ 2, 3, 3, 3, 2, 2, 1, 1, 1, 1 };
    uint64_t used = 0;
    const auto query = [&](const SHL_CONV2D *s, uint64_t sz = 2, uint64_t flags = 0, uint64_t slices = 0, uint64_t tile = 0, uint64_t hint = 0) {
        return shl_conv2d_scalars_tile(context, chain_index, nullptr, nullptr, nullptr, sz, s, flags, slices, &used, tile, hint, nullptr);
    };
    OK(query(&good));
    refused(query(nullptr), "NULL shape");
    for (unsigned f = 0; f < 10; f++)
        for (uint64_t v : { uint64_t(0), uint64_t(1) << 32, uint64_t(1) << 63, ~uint64_t(0) })
        {
            uint64_t fields[10];
            std::memcpy(fields, &good, sizeof(fields));
            fields[f] = v;
            SHL_CONV2D s;
            std::memcpy(&s, fields, sizeof(fields));
            if (f >= 8 && v == 0) // pad 0 is a shape
                OK(query(&s));
            else if ((f == 6 || f == 7) && v) // a stride beyond the image is one output row / column
                OK(query(&s));
            else
                refused(query(&s), "a field of 0 or beyond 32 bits");
        }
    const SHL_CONV2D bad[] = { { 2, 3, 3, 3, 2, 2, 1, 1, 2, 1 },                   // pad_h >= kernel_h
                               { 2, 3, 3, 3, 2, 2, 1, 1, 1, 2 },                   // pad_w >= kernel_w
                               { 2, 1, 3, 3, 4, 2, 1, 1, 1, 1 },                   // height + 2 pad_h < kernel_h
                               { 2, 3, 1, 3, 2, 5, 1, 1, 1, 1 },                   // width + 2 pad_w < kernel_w
                               { 1 << 16, 1 << 8, 1 << 8, 3, 2, 2, 1, 1, 1, 1 },   // C H W >= 2^32
                               { 2, 1 << 8, 1 << 8, 1 << 16, 2, 2, 1, 1, 1, 1 },   // OC OH OW >= 2^32
                               { 1 << 14, 3, 3, 1 << 16, 2, 2, 1, 1, 1, 1 },       // OC inner >= 2^32
                               { 1 << 14, 1 << 8, 1 << 8, 3, 2, 2, 1, 1, 1, 1 } }; // the terms of one launch >= 2^32
    for (const SHL_CONV2D &s : bad)
        refused(query(&s), "a shape outside the contract");
    for (uint64_t sz : { uint64_t(0), uint64_t(17) })
        refused(query(&good, sz), "size");
    for (uint64_t flags : { uint64_t(8), uint64_t(1) << 63 })
        refused(query(&good, 2, flags), "flags");
    for (uint64_t slices : { uint64_t(9), uint64_t(65) })
        refused(query(&good, 2, 0, slices), "more slices than terms, or than 64");
    for (uint64_t tile : { uint64_t(1), uint64_t(2), uint64_t(16), uint64_t(1) << 32 })
        refused(query(&good, 2, 0, 0, tile), "a row tile that is not built");
    for (uint64_t hint : { uint64_t(3), uint64_t(1) << 32 })
        refused(query(&good, 2, 0, 0, 0, hint), "a hint that does not exist");
    {
        Device a(size * 18 * words), r(size * 48 * words), w(3 * 8 * K);
        refused(shl_conv2d_scalars(context, chain_index, w.p, (const uint64_t *)a.p, (uint64_t *)r.p, size, &bad[0], 0, 0, &used), "with operands");
        refused(shl_conv2d_scalars(context, chain_index, w.p, (const uint64_t *)a.p, (uint64_t *)r.p, size, nullptr, 0, 0, &used), "with operands, NULL shape");
    }
    SEALContext_Destroy(context);
    EncParams_Destroy(parms);
    std::printf("conv2d_scalars_asan: %ld launches word for word, %d refusals, no report\n", launches, refusals);
    return 0;
}
