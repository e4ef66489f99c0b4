// The register order of a key-switching key (ntt2_kernels.h), word by word: key_layout_kernel's output for structured and uniform key
// words against 128-bit integer arithmetic, and key_unlayout_kernel's way back.  TEST INFRASTRUCTURE: built by tests/test_ks_keys.py
// against the fiber-emulated library (tests/hipemu/libsealhip_emu.so); `key_layout_check N q_0 ... q_{L-1}` prints "key_layout_check ok".
//
// Why the stored words are checked and not only the key switch's results: ks2 multiplies a raised digit x into a key word w as
// x w - h q with h taken from the stored quotient floor(w 2^64 / q).  A stored quotient that is too small gives the same residue one
// q higher inside the lazy range, so every canonical result stays right - and the headroom of the accumulators (field.h: 4 (n + 1) q)
// is gone, which no parity input shows.  The estimate that key_layout_kernel starts from is exact for almost every uniform word
// (the primes are close to a power of two) and one too small at w = floor(q/2) + 1: the correction loop runs for structured keys only.
#include "context.h"
#include "ntt2_kernels.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace sealhip;
typedef unsigned __int128 u128;

static void ck(hipError_t e, const char *what)
{
    if (e != hipSuccess)
    {
        std::fprintf(stderr, "key_layout_check: %s failed (%d)\n", what, (int)e);
        std::exit(2);
    }
}

int main(int argc, char **argv)
{
    if (argc < 4)
    {
        std::fprintf(stderr, "usage: key_layout_check N q_0 ... q_{L-1}\n");
        return 2;
    }
    const size_t N = std::strtoull(argv[1], nullptr, 10);
    std::vector<uint64_t> primes;
    for (int i = 2; i < argc; i++)
        primes.push_back(std::strtoull(argv[i], nullptr, 10));
    const unsigned L = (unsigned)primes.size();
    const size_t digits = L - 1;
    Context ctx(Scheme::ckks, N, primes, 0, true);
    const NttTables &t = ctx.ntt_tables();
    if (!t.fp_host || ((size_t)1 << t.log_n) != N)
    {
        std::fprintf(stderr, "key_layout_check: no class table for this context\n");
        return 2;
    }
    const size_t nat_words = digits * 2 * L * N, reg_words = key_register_order_words(t, L, digits);
    uint64_t *d_in, *d_out, *d_back;
    ck(hipMalloc((void **)&d_in, nat_words * 8), "hipMalloc");
    ck(hipMalloc((void **)&d_out, reg_words * 8), "hipMalloc");
    ck(hipMalloc((void **)&d_back, nat_words * 8), "hipMalloc");
    std::vector<uint64_t> in(nat_words), out(reg_words), back(nat_words);
    std::mt19937_64 rng(12345);
    const char *patterns[] = { "qm1", "half", "half1", "alt", "mix4", "one", "zero", "uniform" };
    size_t pairs = 0, doubles = 0, corrected = 0;
    unsigned n_int = 0, n_fp = 0;
    for (const char *pat : patterns)
    {
        for (size_t j = 0; j < digits; j++)
            for (unsigned k = 0; k < 2; k++)
                for (unsigned c = 0; c < L; c++)
                {
                    const uint64_t q = primes[c];
                    const uint64_t edge[4] = { 0, q - 1, q / 2, q / 2 + 1 };
                    uint64_t *w = in.data() + ((j * 2 + k) * L + c) * N;
                    for (size_t i = 0; i < N; i++)
                        w[i] = !std::strcmp(pat, "qm1")     ? q - 1
                               : !std::strcmp(pat, "half")  ? q / 2
                               : !std::strcmp(pat, "half1") ? q / 2 + 1
                               : !std::strcmp(pat, "alt")   ? ((i & 1) ? q - 1 : 0)
                               : !std::strcmp(pat, "mix4")  ? edge[rng() & 3]
                               : !std::strcmp(pat, "one")   ? 1
                               : !std::strcmp(pat, "zero")  ? 0
                                                            : rng() % q;
                }
        ck(hipMemcpy(d_in, in.data(), nat_words * 8, hipMemcpyHostToDevice), "upload");
        ck(hipMemset(d_out, 0xff, reg_words * 8), "fill");
        ck(key_to_register_order(t, d_in, d_out, L, digits, 0), "key_to_register_order");
        ck(key_from_register_order(t, d_out, d_back, L, digits, 0), "key_from_register_order");
        ck(hipDeviceSynchronize(), "synchronize");
        ck(hipMemcpy(out.data(), d_out, reg_words * 8, hipMemcpyDeviceToHost), "download");
        ck(hipMemcpy(back.data(), d_back, nat_words * 8, hipMemcpyDeviceToHost), "download");
        n_int = n_fp = 0;
        for (size_t j = 0; j < digits; j++)
            for (unsigned c = 0; c < L; c++)
            {
                const uint64_t q = primes[c];
                const bool fp = t.fp_host[c] != 0;
                (fp ? n_fp : n_int)++;
                const uint64_t *o = out.data() + ((j * key_digit_units(t, L) + key_comp_offset_units(t, c)) << t.log_n);
                for (unsigned k = 0; k < 2; k++)
                    for (size_t p = 0; p < N; p++)
                    {
                        // register position p = hg*4096 + e*256 + tid  <->  natural hg*4096 + (tid>>4)*256 + (tid&15)*16 + e
                        const size_t hg = p >> 12, e = (p >> 8) & 15, tid = p & 255;
                        const size_t nat = (hg << 12) + ((tid >> 4) << 8) + ((tid & 15) << 4) + e;
                        const uint64_t w = in[((j * 2 + k) * L + c) * N + nat];
                        if (fp)
                        {
                            // balanced representative in (-q/2, q/2]
                            double d;
                            std::memcpy(&d, &o[2 * p + k], 8);
                            const double want = w > q / 2 ? -(double)(q - w) : (double)w;
                            if (!(d == want) || !(2 * d <= (double)q && 2 * d > -(double)q))
                            {
                                std::fprintf(stderr, "key_layout_check: %s: digit %zu poly %u prime %u (q = %llu) position %zu: word %llu stored as %.17g, expected %.17g\n",
                                             pat, j, k, c, (unsigned long long)q, p, (unsigned long long)w, d, want);
                                return 1;
                            }
                            doubles++;
                        }
                        else
                        {
                            const uint64_t *pr = o + ((size_t)k << (t.log_n + 1)) + 2 * p;
                            const uint64_t quot = (uint64_t)(((u128)w << 64) / q);
                            if (pr[0] != w || pr[1] != quot)
                            {
                                std::fprintf(stderr, "key_layout_check: %s: digit %zu poly %u prime %u (q = %llu) position %zu: word %llu stored as (%llu, %llu), expected quotient floor(w 2^64 / q) = %llu\n",
                                             pat, j, k, c, (unsigned long long)q, p, (unsigned long long)w, (unsigned long long)pr[0],
                                             (unsigned long long)pr[1], (unsigned long long)quot);
                                return 1;
                            }
                            // how often the estimate from floor(2^128 / q) alone would have been short (the correction loop's work)
                            const u128 ratio = ~(u128)0 / q; // q is odd and above 2: floor((2^128 - 1) / q) == floor(2^128 / q)
                            const uint64_t r_hi = (uint64_t)(ratio >> 64), r_lo = (uint64_t)ratio;
                            const u128 est = (u128)w * r_hi + (((u128)w * r_lo) >> 64);
                            corrected += (uint64_t)est != quot;
                            pairs++;
                        }
                    }
            }
        if (std::memcmp(back.data(), in.data(), nat_words * 8))
        {
            size_t i = 0;
            while (back[i] == in[i])
                i++;
            std::fprintf(stderr, "key_layout_check: %s: natural order -> register order -> natural order differs first at word %zu: %llu, was %llu\n", pat,
                         i, (unsigned long long)back[i], (unsigned long long)in[i]);
            return 1;
        }
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_back);
    if (!n_int || !n_fp || !corrected)
    {
        std::fprintf(stderr, "key_layout_check: the chain must reach both classes and the correction loop (%u integer, %u double-precision components, %zu corrected quotients)\n",
                     n_int, n_fp, corrected);
        return 1;
    }
    std::printf("key_layout_check ok: %zu pairs (%zu quotients beyond the estimate), %zu balanced doubles\n", pairs, corrected, doubles);
    return 0;
}
