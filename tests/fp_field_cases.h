// TEST ONLY: the case body shared by the host check (tests/field_check.cpp, g++ against tests/hipemu's stand-in hip_runtime.h)
// and the device check (tests/device_fp_field_check.hip, hipcc for gfx950) of the double-precision back end Field<true>
// (seal_amd/csrc/field.h) and of the templates of seal_amd/csrc/ntt2_device.h that place its range reductions.
//
// One call of fpcases::run_round() is one (prime, thread, round): operands come from a seeded xorshift and are steered to where
// the bounds of field.h are tight - products on (k + 1/2) q, magnitudes on the documented ladder, values at +-1.80 q entering the
// pack -, every result is compared with 128-bit integer arithmetic or with a bound written out from field.h's own formulas, and
// fp_to_bits of every double produced is folded into an order-independent digest.  IEEE-754 with FMA and round-to-nearest-even
// fixes every one of those bits, so the host's and the device's digests of the same streams are equal unless the code generation
// differs (contraction, rounding mode, conversions).
//
// Check codes (Sink::code = the highest that failed; Sink::first = code, q and two operand words of the first failure):
//    1 balanced product: not an integer / residue      2 balanced product: |r| > q (0.5 + 0.1875 |x| / q) + 2
//    3 w in {0, +-1, +-floor(q/2)}                      4 unbalanced product: residue / 0.875 q / fp_to_canon of it
//    5 two32 product, fp_from_u64                       6 fp_fix: residue / magnitude
//    7 fp_to_canon at its edges                         8 fp_from_u52
//   10 CKKS tensor product                             11 tail pass 1: fp_mulmod(v, pinv) + u
//   12 tail pass 2: the rounding epilogue              13 map_src<true>
//   20 forward stage: residue                          21 forward stage: magnitude >= 2^53
//   22 forward stage: magnitude above the ladder       23 a schedule whose documented bound is not below 2^53
//   24 phase template differs from the staged run      25 phase template: residue
//   26 pass-1 / pass-2 crossing not below 2^51         27 crossing above 1.80 q
//   30 inverse phase: residue                          31 inverse phase: magnitude
//   32 last inverse stage: residue                     33 last inverse stage: magnitude
//   40 unpack52(pack52(x)) != x
//   50 accumulator: running sum >= 2^53                51 accumulator: running sum above its bound
//   52 acc_to_canon                                    53 accumulator schedule whose documented bound is not below 2^53
#pragma once
#include "ntt2_device.h"
#include <cstdio>
#include <string>

// the case body's copy of the kernels' schedules (mutants (c) and (d) of profiles/fp_field_check.txt change these)
#ifndef FPC_LEAN_FIX1
#define FPC_LEAN_FIX1 2 // p1_tile, LEAN: phase_fwd_fix<FP, 4, 2> in phase B
#endif
#ifndef FPC_ACC_RUN
#define FPC_ACC_RUN 7 // ks2: acc_fix when (J - j0) % 7 == 6
#endif

namespace fpcases
{
    using namespace sealhip;
    typedef unsigned __int128 u128;
    typedef __int128 i128;

    constexpr double kTwo53 = 9007199254740992.0, kTwo51 = 2251799813685248.0;
    constexpr double kLeanEntryQ = 1.13; // ntt2_kernels.hip, kLeanEntry
    constexpr int kMaxSlots = 24;
    // slots of Sink::maxq: 1..7 forward stages after a fix (largest magnitude reached when every stage starts from the largest
    // seen so far), 8 the crossing, 9 the lean run's exit, 12 the sums and differences entering the last inverse stage (units of
    // 2 q), 13 a four-stage inverse phase's exit, 14 the last inverse stage, 15 accumulator (FPC_ACC_RUN terms), 16 accumulator
    // with 8 terms between two acc_fix (measured headroom, not asserted)
    constexpr int kSlotCross = 8, kSlotLeanOut = 9, kSlotInv = 9, kSlotInvLast = 14, kSlotAcc = 15, kSlotAcc8 = 16;

    constexpr unsigned kNumPrimes = 9;
    constexpr unsigned kUniTw = 64; // wave-uniform twiddles per prime
    inline const uint64_t *primes()
    {
        // the seven of tests/field_check.cpp, the largest prime = 1 (mod 2^17) below 2^50, and 65537
        static const uint64_t qs[kNumPrimes] = { (1ull << 50) - (1ull << 17) * 3 + 1, (1ull << 49) + (1ull << 17) + 1, (1ull << 40) + (1ull << 17) * 7 + 1,
                                                 (1ull << 30) - (1ull << 17) + 1,     (1ull << 20) + 1,                1125899906826241ull,
                                                 1125899906629633ull,                 (1ull << 50) - (1ull << 17) * 23 + 1, 65537ull };
        return qs;
    }
    inline FpDesc make_desc(uint64_t q)
    {
        return FpDesc{ (double)q, 1.0 / (double)q, (double)((1ull << 32) % q), q };
    }

    struct Rng
    {
        uint64_t s;
        SHL_HD uint64_t next()
        {
            s ^= s << 13;
            s ^= s >> 7;
            s ^= s << 17;
            return s * 0x2545F4914F6CDD1Dull;
        }
    };
    SHL_HD uint64_t seed_of(unsigned prime, unsigned thread, unsigned round)
    {
        return 0x9E3779B97F4A7C15ull * ((uint64_t)thread * 4096 + round + 1) + prime;
    }
    // the wave-uniform twiddle table of a prime: balanced, the extremes first
    inline void fill_uniform_tw(uint64_t q, unsigned prime, double *tab)
    {
        Rng r{ 88172645463325252ull + prime };
        const int64_t h = (int64_t)(q / 2);
        for (unsigned i = 0; i < kUniTw; i++)
        {
            const uint64_t v = r.next();
            int64_t w = (int64_t)(v % q);
            w = w > h ? w - (int64_t)q : w;
            if (i < 8)
                w = (i & 1 ? -1 : 1) * (h - (int64_t)(i >> 1));
            else if (i < 12)
                w = (i & 1 ? -1 : 1) * (int64_t)(1 + (i >> 1 & 1));
            tab[i] = (double)w;
        }
    }

    struct Sink
    {
        uint64_t fails, code, first[4], digest, maxq[kMaxSlots];
        bool fold;
        SHL_HD void fail(unsigned c, uint64_t q, uint64_t a, uint64_t b)
        {
            if (!fails)
            {
                first[0] = c;
                first[1] = q;
                first[2] = a;
                first[3] = b;
            }
            fails++;
            code = c > code ? c : code;
        }
        SHL_HD void word(uint64_t b)
        {
            if (fold)
            {
                b ^= b >> 31;
                b *= 0x9FB21C651E98DF25ull;
                b ^= b >> 29;
                digest += b; // a wrapping sum of mixed words: independent of the order the threads arrive in
            }
        }
        SHL_HD double out(double d)
        {
            word(fp_to_bits(d));
            return d;
        }
        SHL_HD void mag(int slot, double units_of_q)
        {
            const uint64_t b = fp_to_bits(units_of_q); // non-negative doubles order as their bit patterns
            maxq[slot] = b > maxq[slot] ? b : maxq[slot];
        }
    };
    SHL_HD Sink sink_zero(bool fold)
    {
        Sink s;
        s.fails = s.code = s.digest = 0;
        for (int i = 0; i < 4; i++)
            s.first[i] = 0;
        for (int i = 0; i < kMaxSlots; i++)
            s.maxq[i] = 0;
        s.fold = fold;
        return s;
    }
    // what a whole run leaves behind for one prime (the device check's only output buffer)
    struct Result
    {
        unsigned long long fails, code, claimed, first[4], digest, maxq[kMaxSlots];
    };
    SHL_HD void merge(Result &r, const Sink &s)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        if (s.fails)
        {
            atomicAdd(&r.fails, (unsigned long long)s.fails);
            atomicMax(&r.code, (unsigned long long)s.code);
            if (atomicCAS(&r.claimed, 0ull, 1ull) == 0ull)
                for (int i = 0; i < 4; i++)
                    r.first[i] = s.first[i];
        }
        if (s.digest)
            atomicAdd(&r.digest, (unsigned long long)s.digest);
        for (int i = 0; i < kMaxSlots; i++)
            if (s.maxq[i])
                atomicMax(&r.maxq[i], (unsigned long long)s.maxq[i]);
#else
        if (s.fails)
        {
            if (!r.claimed)
                for (int i = 0; i < 4; i++)
                    r.first[i] = s.first[i];
            r.claimed = 1;
            r.fails += s.fails;
            r.code = s.code > r.code ? s.code : r.code;
        }
        r.digest += s.digest;
        for (int i = 0; i < kMaxSlots; i++)
            r.maxq[i] = s.maxq[i] > r.maxq[i] ? s.maxq[i] : r.maxq[i];
#endif
    }

#define FPC_EXPECT(cond, c, a, b)                              \
    do                                                         \
    {                                                          \
        if (!(cond))                                           \
            sk.fail((c), m.qi, (uint64_t)(a), (uint64_t)(b));  \
    } while (0)

    // ---- the integer side
    // (128-bit division is a long routine on the device: one copy, not one per use)
    __host__ __device__ __attribute__((noinline)) inline uint64_t umod128(u128 v, uint64_t q)
    {
        return (uint64_t)(v % q);
    }
    __host__ __device__ __attribute__((noinline)) inline uint64_t udiv128(u128 v, uint64_t d)
    {
        return (uint64_t)(v / d);
    }
    SHL_HD double fabs_(double v)
    {
        return v < 0.0 ? -v : v;
    }
    SHL_HD bool is_int53(double v)
    {
        return fabs_(v) < kTwo53 && (double)(int64_t)v == v;
    }
    // integer-valued |v| < 2^63 -> [0, q)
    SHL_HD uint64_t canon(double v, uint64_t q)
    {
        const int64_t r = (int64_t)v % (int64_t)q;
        return (uint64_t)(r < 0 ? r + (int64_t)q : r);
    }
    SHL_HD uint64_t mulq(uint64_t a, uint64_t b, uint64_t q)
    {
        return umod128((u128)a * b, q);
    }
    SHL_HD uint64_t addq(uint64_t a, uint64_t b, uint64_t q)
    {
        const uint64_t s = a + b;
        return s >= q ? s - q : s;
    }
    SHL_HD uint64_t subq(uint64_t a, uint64_t b, uint64_t q)
    {
        return a >= b ? a - b : a + q - b;
    }
    // uniform in [-floor(q/2), floor(q/2)]
    SHL_HD double balanced(uint64_t v, uint64_t q)
    {
        const uint64_t r = v % q;
        return r > q / 2 ? -(double)(q - r) : (double)r;
    }
    // the integer nearest to (k + 1/2) q / d
    SHL_HD uint64_t tie_point(uint64_t k, uint64_t q, uint64_t d)
    {
        return udiv128((u128)(2 * k + 1) * q + d, 2 * d);
    }
    // B -> 1.1875 B + 0.5, `stages` times (field.h)
    SHL_HD double ladder(double b, int stages)
    {
        for (int s = 0; s < stages; s++)
            b = 1.1875 * b + 0.5;
        return b;
    }
    // floor(b q) as an exact double (b q < 2^53)
    SHL_HD double units(double b, const FpDesc &m)
    {
        return (double)(int64_t)(b * m.q);
    }

    // ---- primitives
    SHL_HD void prim_cases(const FpDesc &m, Rng &rng, unsigned it, Sink &sk)
    {
        const uint64_t q = m.qi, h = q / 2;
        const double qd = m.q;
        // balanced multiplier, x on the ties of the rounding: (k + 1/2) q / |w| and its neighbours, |x| up to the ladder's values
        for (int rep = 0; rep < 4; rep++)
        {
            const double B = ladder(0.5, (int)((it + rep) & 7));
            const uint64_t xmax = (uint64_t)units(B, m);
            const uint64_t v = rng.next();
            uint64_t wa;
            switch ((it + rep) % 3)
            {
            case 0: wa = 1 + v % h; break;
            case 1: wa = 1 + v % (h < 16 ? h : 16); break; // small multipliers: the product lands within |w| / 2 of the tie
            default: wa = h - (v & 7); break;
            }
            // k with (k + 1/2) q / wa <= xmax
            const uint64_t kmax = udiv128((u128)xmax * wa, q);
            const uint64_t kk = kmax ? ((v >> 8) & 1 ? kmax - 1 - ((v >> 9) & 3) % kmax : (rng.next() >> 11) % kmax) : 0;
            uint64_t xa = tie_point(kk, q, wa) + ((v >> 16) % 3) - 1;
            xa = xa > xmax ? xmax : xa;
            const double x = (v >> 20) & 1 ? -(double)xa : (double)xa, w = (v >> 21) & 1 ? -(double)wa : (double)wa;
            const double r = sk.out(fp_mulmod(x, w, m.q, m.qinv));
            FPC_EXPECT(is_int53(r) && canon(r, q) == mulq(canon(x, q), canon(w, q), q), 1u, fp_to_bits(x), fp_to_bits(w));
            FPC_EXPECT(fabs_(r) <= qd * (0.5 + 0.1875 * fabs_(x) / qd) + 2.0, 2u, fp_to_bits(x), fp_to_bits(w));
        }
        // w in {0, +-1, +-floor(q/2)}
        {
            const uint64_t v = rng.next();
            const double ws[5] = { 0.0, 1.0, -1.0, (double)h, -(double)h };
            const double xa = (v & 1) ? units(7.88, m) - (double)((v >> 1) & 1023) : (double)(int64_t)((v >> 11) % (uint64_t)units(7.88, m));
            const double x = (v & 2048) ? -xa : xa;
            for (int i = 0; i < 5; i++)
            {
                const double r = sk.out(fp_mulmod(x, ws[i], m.q, m.qinv));
                FPC_EXPECT(is_int53(r) && canon(r, q) == mulq(canon(x, q), canon(ws[i], q), q) && fabs_(r) <= qd * (0.5 + 0.1875 * fabs_(x) / qd) + 2.0, 3u,
                           fp_to_bits(x), fp_to_bits(ws[i]));
            }
        }
        // the unbalanced use: x, w in [0, q)
        for (int rep = 0; rep < 2; rep++)
        {
            const uint64_t v = rng.next();
            uint64_t wa = (v & 3) == 0 ? q - 1 - ((v >> 2) & 3) : 1 + (v >> 4) % (q - 1), xa;
            if ((v >> 60) & 1)
            {
                const uint64_t kmax = udiv128((u128)(q - 1) * wa, q); // (k + 1/2) q / wa < q
                xa = tie_point(kmax ? (rng.next() >> 11) % kmax : 0, q, wa) + ((v >> 61) & 1);
                xa = xa >= q ? q - 1 : xa;
            }
            else
                xa = (v >> 62) ? q - 1 : rng.next() % q;
            const double r = sk.out(fp_mulmod((double)xa, (double)wa, m.q, m.qinv));
            const uint64_t ref = mulq(xa, wa, q);
            FPC_EXPECT(is_int53(r) && canon(r, q) == ref && fabs_(r) <= 0.875 * qd && fp_to_canon(r, m) == ref, 4u, xa, wa);
        }
        // 2^32 mod q as the multiplier of a 32-bit word, and the conversion built on it
        {
            const uint64_t v = rng.next();
            const uint32_t his[4] = { 0u, 1u, 0xffffffffu, (uint32_t)(v >> 32) };
            for (int i = 0; i < 4; i++)
            {
                const double hi = (double)his[i];
                const double r = sk.out(fp_mulmod(hi, m.two32, m.q, m.qinv));
                FPC_EXPECT(is_int53(r) && canon(r, q) == mulq(his[i], (uint64_t)m.two32, q) && fabs_(r) <= qd * (0.5 + 0.375 * hi * m.two32 / (qd * qd)) + 2.0, 5u,
                           his[i], (uint64_t)m.two32);
            }
            const uint64_t xs[4] = { ~0ull, (v << 32) | 0xffffffffull, 0xffffffffull, rng.next() };
            for (int i = 0; i < 4; i++)
            {
                const double a = sk.out(fp_from_u64(xs[i], m));
                FPC_EXPECT(is_int53(a) && canon(a, q) == xs[i] % q && fabs_(a) < qd + 4294967296.0, 5u, xs[i], fp_to_bits(a));
            }
        }
        // fp_fix on the ties +-(k + 1/2) q and next to 2^53.  k = rint(fl(x qinv)) is within 1/2 + 2^-52 |x| / q (1 + 2^-50) of
        // x / q (two roundings), so |x - k q| <= q / 2 + 2^-52 |x| + 1
        {
            const uint64_t v = rng.next();
            const uint64_t kmax = (uint64_t)(kTwo53 / qd) - 1; // (kmax + 1/2) q < 2^53
            const uint64_t kk = (v & 1) ? kmax - ((v >> 1) & 7) % (kmax + 1) : (v >> 11) % (kmax + 1);
            const uint64_t tie = (uint64_t)(((u128)(2 * kk + 1) * q) >> 1); // floor((k + 1/2) q); + 1 = the other side of the tie
            const double xs[4] = { (double)tie, -(double)(tie + 1), kTwo53 - 1.0 - (double)((v >> 20) & 1023), -(kTwo53 - 1.0 - (double)((v >> 30) & 1023)) };
            for (int i = 0; i < 4; i++)
            {
                const double f = sk.out(fp_fix(xs[i], m.q, m.qinv));
                FPC_EXPECT(is_int53(f) && canon(f, q) == canon(xs[i], q), 6u, fp_to_bits(xs[i]), fp_to_bits(f));
                FPC_EXPECT(fabs_(f) <= 0.5 * qd + fabs_(xs[i]) * 2.220446049250313e-16 + 1.0, 6u, fp_to_bits(xs[i]), fp_to_bits(f));
            }
        }
        // conversions at their edges
        {
            const double xs[6] = { 0.0, -0.0, 1.0, -1.0, (double)(q - 1), -(double)(q - 1) };
            const uint64_t want[6] = { 0, 0, 1, q - 1, q - 1, 1 };
            for (int i = 0; i < 6; i++)
            {
                const uint64_t c = fp_to_canon(xs[i], m);
                sk.word(c);
                FPC_EXPECT(c == want[i], 7u, fp_to_bits(xs[i]), c);
            }
            const uint64_t us[3] = { 0ull, (1ull << 52) - 1, rng.next() >> 12 };
            for (int i = 0; i < 3; i++)
            {
                const double d = sk.out(fp_from_u52(us[i]));
                FPC_EXPECT(d == (double)us[i] && (uint64_t)d == us[i], 8u, us[i], fp_to_bits(d));
            }
        }
    }

    // ---- the kernels' own expressions
    SHL_HD uint64_t pick_canon(uint64_t v, uint64_t q)
    {
        switch (v & 7)
        {
        case 0: return q - 1;
        case 1: return 0;
        case 2: return q / 2 + ((v >> 3) & 1);
        default: return (v >> 4) % q;
        }
    }
    SHL_HD void use_site_cases(const FpDesc &m, Rng &rng, unsigned it, Sink &sk)
    {
        const uint64_t q = m.qi;
        const double qd = m.q;
        // the 2 x 2 tensor product (poly_kernels.hip, ckks_multiply_2x2_kernel)
        {
            const uint64_t x0 = pick_canon(rng.next(), q), x1 = pick_canon(rng.next(), q), y0 = pick_canon(rng.next(), q), y1 = pick_canon(rng.next(), q);
            const double a0 = fp_from_u52(x0), a1 = fp_from_u52(x1), b0 = fp_from_u52(y0), b1 = fp_from_u52(y1);
            const double r00 = sk.out(fp_mulmod(a0, b0, m.q, m.qinv)), r11 = sk.out(fp_mulmod(a1, b1, m.q, m.qinv));
            const double mid = sk.out(fp_mulmod(a0, b1, m.q, m.qinv) + fp_mulmod(a1, b0, m.q, m.qinv));
            const uint64_t o0 = fp_to_canon(r00, m), o1 = fp_to_canon(fp_fix(mid, m.q, m.qinv), m), o2 = fp_to_canon(r11, m);
            FPC_EXPECT(o0 == mulq(x0, y0, q) && o2 == mulq(x1, y1, q), 10u, x0, y0);
            FPC_EXPECT(o1 == addq(mulq(x0, y1, q), mulq(x1, y0, q), q) && fabs_(mid) <= 1.75 * qd, 10u, x0, x1);
        }
        // tail pass 1 (ntt2_kernels.hip, tail2_p1_body): x = fp_mulmod(v, pinv) + u, v = from_any(r1) + f1, one fix
        {
            const uint64_t v0 = rng.next();
            const uint64_t r1 = (v0 & 3) == 0 ? ~0ull : (v0 & 3) == 1 ? (rng.next() | 0xffffffffull) : rng.next();
            const uint64_t f1c = pick_canon(rng.next(), q), f2c = pick_canon(rng.next(), q);
            const bool u_small = (v0 >> 2) & 1;
            const uint64_t r2 = u_small ? ((v0 >> 3) & 1 ? (1ull << 52) - 1 : rng.next() >> 12) : ((v0 >> 3) & 1 ? ~0ull : rng.next());
            const uint64_t pw = (v0 >> 4) & 1 ? q / 2 + ((v0 >> 5) & 1) : 1 + rng.next() % (q - 1);
            const double pinv = pw > q / 2 ? -(double)(q - pw) : (double)pw;
            const double f1 = fp_from_u52(f1c), f2 = fp_from_u52(f2c);
            const double v = sk.out(Field<true>::from_any(r1, m) + f1), u = sk.out((u_small ? fp_from_u52(r2) : Field<true>::from_any(r2, m)) + f2);
            double x = sk.out(fp_mulmod(v, pinv, m.q, m.qinv) + u);
            const double pre = x;
            Field<true>::fix(x, m);
            sk.out(x);
            const uint64_t ref = addq(mulq(addq(r1 % q, f1c, q), pw, q), addq(r2 % q, f2c, q), q);
            FPC_EXPECT(is_int53(pre) && is_int53(x) && canon(x, q) == ref && fabs_(x) <= 0.5 * qd + fabs_(pre) * 2.220446049250313e-16 + 1.0, 11u, r1, r2);
        }
        // tail pass 2 (tail2_p2_body): fp_to_canon(fp_fix(fp_mulmod(s - t, mul))), s = S P^-1 + c or the folded word
        {
            const uint64_t v0 = rng.next();
            const uint64_t av = pick_canon(rng.next(), q), cv = pick_canon(rng.next(), q);
            const uint64_t pw = (v0 & 1) ? q / 2 + ((v0 >> 1) & 1) : 1 + rng.next() % (q - 1), mw = (v0 & 4) ? q / 2 + ((v0 >> 3) & 1) : 1 + rng.next() % (q - 1);
            const double pm_fp = pw > q / 2 ? -(double)(q - pw) : (double)pw, mul_fp = mw > q / 2 ? -(double)(q - mw) : (double)mw;
            const double t = (v0 & 16) ? ((v0 & 32) ? 1.0 : -1.0) * (double)(q / 2) : balanced(rng.next(), q);
            const bool folded = (v0 >> 6) & 1;
            const double s = sk.out(folded ? fp_from_u52(av) : fp_mulmod(fp_from_u52(av), pm_fp, m.q, m.qinv) + fp_from_u52(cv));
            const double r = sk.out(fp_mulmod(s - t, mul_fp, m.q, m.qinv));
            const uint64_t o = fp_to_canon(sk.out(fp_fix(r, m.q, m.qinv)), m);
            const uint64_t sref = folded ? av : addq(mulq(av, pw, q), cv, q);
            FPC_EXPECT(o == mulq(subq(sref, canon(t, q), q), mw, q), 12u, av, cv);
        }
        // map_src<true> in its four modes, the source word at the ends of its range
        {
            const uint64_t v0 = rng.next();
            const uint64_t sqs[4] = { q, (1ull << 60) - (1ull << 18) + 1, (1ull << 50) + (1ull << 17) + 1, 786433ull };
            const uint64_t src_q = sqs[(v0 >> 8) & 3], half = src_q >> 1, fix = pick_canon(rng.next(), q);
            for (int mode = 0; mode < 4; mode++)
            {
                const uint64_t top = mode == 0 ? q : (mode == 2 ? src_q : 0); // exclusive bound of the source word, 0 = any word
                uint64_t v;
                switch ((it + mode) % 6)
                {
                case 0: v = 0; break;
                case 1: v = half - 1; break;
                case 2: v = half; break;
                case 3: v = src_q - 1; break;
                case 4: v = ~0ull; break;
                default: v = rng.next(); break;
                }
                if (top && v >= top)
                    v = mode == 0 ? v % q : top - 1;
                const SrcMap s{ mode, half, src_q, fix };
                const double x = sk.out(map_src<true>(v, s, m));
                const uint64_t r = mode == 3 ? v : (v + half >= src_q ? v + half - src_q : v + half);
                const uint64_t ref = mode <= 1 ? v % q : addq(r % q, fix, q);
                const double bound = mode == 0 ? qd - 1.0 : mode == 1 ? qd + 4294967296.0 : 0.5 * qd + 2.0;
                FPC_EXPECT(is_int53(x) && canon(x, q) == ref && fabs_(x) <= bound, 13u, v, (uint64_t)mode << 60 | (src_q & 0xfffffffffffffffull));
            }
        }
    }

    // ---- chains through the templates of ntt2_device.h
    // twiddles: even stages take theirs from the wave-uniform table (ld_uniform: the scalar path on the device), odd stages from
    // per-lane values; `ub` is the same in every lane of a workgroup
    struct TwSet
    {
        const double *utab;
        unsigned ub;
        double lane[16];
        SHL_HD double get(int stage, int g) const
        {
            if (stage & 1)
                return lane[(stage * 5 + g) & 15];
            return ld_uniform(utab, (ub + (unsigned)stage * 8u + (unsigned)g) & (kUniTw - 1));
        }
    };
    SHL_HD void fill_lane_tw(TwSet &tw, const FpDesc &m, Rng &rng)
    {
        const uint64_t q = m.qi, h = q / 2;
        for (int i = 0; i < 16; i++)
        {
            const uint64_t v = rng.next();
            tw.lane[i] = (v & 3) == 0 ? ((v & 4) ? -1.0 : 1.0) * (double)(h - ((v >> 3) & 7)) : (v & 3) == 1 ? ((v & 4) ? -1.0 : 1.0) * (double)(1 + ((v >> 3) & 3)) : balanced(v >> 5, q);
        }
    }
    // reference stages on canonical residues
    SHL_HD void ref_stage_fwd(uint64_t (&r)[16], int bit, const TwSet &tw, int stage, uint64_t q)
    {
        for (int g = 0; g < (8 >> bit); g++)
        {
            const uint64_t w = canon(tw.get(stage, g), q);
            for (int k = 0; k < (1 << bit); k++)
            {
                const int e0 = (g << (bit + 1)) | k, e1 = e0 | (1 << bit);
                const uint64_t t = mulq(r[e1], w, q), a = r[e0];
                r[e0] = addq(a, t, q);
                r[e1] = subq(a, t, q);
            }
        }
    }
    SHL_HD void ref_stage_inv(uint64_t (&r)[16], int bit, const TwSet &tw, int stage, uint64_t q)
    {
        for (int g = 0; g < (8 >> bit); g++)
        {
            const uint64_t w = canon(tw.get(stage, g), q);
            for (int k = 0; k < (1 << bit); k++)
            {
                const int e0 = (g << (bit + 1)) | k, e1 = e0 | (1 << bit);
                const uint64_t a = r[e0], b = r[e1];
                r[e0] = addq(a, b, q);
                r[e1] = mulq(subq(a, b, q), w, q);
            }
        }
    }
    // one forward stage (stage_fwd<true, BIT>) of the staged run; `stage` numbers the twiddle set
    template <int BIT>
    SHL_HD void one_stage(double (&x)[16], const FpDesc &m, const TwSet &tw, int stage)
    {
        stage_fwd<true, BIT>(x, m, [&](int g) { return tw.get(stage, g); });
    }
    SHL_HD void stage_by_bit(double (&x)[16], const FpDesc &m, const TwSet &tw, int stage)
    {
        switch (stage & 3)
        {
        case 0: one_stage<3>(x, m, tw, stage); break;
        case 1: one_stage<2>(x, m, tw, stage); break;
        case 2: one_stage<1>(x, m, tw, stage); break;
        default: one_stage<0>(x, m, tw, stage); break;
        }
    }
    SHL_HD void fix_all(double (&x)[16], const FpDesc &m)
    {
        for (int a = 0; a < 16; a++)
            Field<true>::fix(x[a], m);
    }
    // after a stage: residues, 2^53, the ladder; returns the largest magnitude
    SHL_HD double check_regs(const double (&x)[16], const uint64_t (&ref)[16], double bound_q, const FpDesc &m, Sink &sk, unsigned c_res, unsigned c_53, unsigned c_lad,
                             uint64_t tag)
    {
        double mx = 0.0;
        for (int a = 0; a < 16; a++)
        {
            sk.out(x[a]);
            const double v = fabs_(x[a]);
            mx = v > mx ? v : mx;
            FPC_EXPECT(v < kTwo53, c_53, fp_to_bits(x[a]), tag);
            FPC_EXPECT(is_int53(x[a]) && canon(x[a], m.qi) == ref[a], c_res, fp_to_bits(x[a]), tag);
            FPC_EXPECT(v <= bound_q * m.q + 2.0, c_lad, fp_to_bits(x[a]), tag);
        }
        return mx;
    }
    // Stage by stage from a fixed value (entry_q = 0.5) or an unfixed digit (kLeanEntryQ): every register of a stage starts at
    // +-(the magnitude `seed` gives), the sign of each second operand chosen so that its product adds to the first.
    // LADDER_SEED = false: the largest magnitude any earlier stage of this run produced (what the arithmetic reaches: recorded);
    // true: the documented bound of the stage before (each stage's bound has to carry the next one's - the check that fails when
    // a reduction comes one stage too late).
    template <bool LADDER_SEED>
    SHL_HD void staged_growth(const FpDesc &m, const TwSet &tw, Rng &rng, double entry_q, int stages, Sink &sk)
    {
        const uint64_t q = m.qi;
        double seen = units(entry_q, m);
        for (int s = 0; s < stages; s++)
        {
            const double in_q = ladder(entry_q, s), out_q = ladder(entry_q, s + 1);
            FPC_EXPECT(out_q * m.q + 2.0 < kTwo53, 23u, (uint64_t)s, fp_to_bits(out_q));
            const double mag = LADDER_SEED ? units(in_q, m) : seen;
            double x[16];
            uint64_t ref[16];
            const int bit = 3 - (s & 3);
            const uint64_t v = rng.next();
            for (int g = 0; g < (8 >> bit); g++)
            {
                // the product's sign with a positive second operand (fp_mulmod is odd in x)
                const double probe = fp_mulmod(mag, tw.get(s, g), m.q, m.qinv);
                for (int k = 0; k < (1 << bit); k++)
                {
                    const int e0 = (g << (bit + 1)) | k, e1 = e0 | (1 << bit);
                    const bool neg = (v >> e0) & 1, diff = (v >> (16 + e0)) & 1; // grow the sum or the difference
                    x[e0] = neg ? -mag : mag;
                    x[e1] = ((probe < 0.0) != neg) != diff ? -mag : mag;
                }
            }
            for (int a = 0; a < 16; a++)
                ref[a] = canon(x[a], q);
            stage_by_bit(x, m, tw, s);
            ref_stage_fwd(ref, bit, tw, s, q);
            const double mx = check_regs(x, ref, out_q, m, sk, 20u, 21u, 22u, (uint64_t)s << 8 | (LADDER_SEED ? 1 : 0));
            seen = mx > seen && mx < kTwo53 ? mx : seen;
            if (!LADDER_SEED && entry_q == 0.5)
                sk.mag(1 + s, seen / m.q);
        }
    }

    template <int FIXAT>
    SHL_HD void phase_fix_case(double (&x)[16], double (&y)[16], const FpDesc &m, const TwSet &tw, int s0)
    {
        phase_fwd_fix<true, 4, FIXAT>(x, m, [&](int t, int g) { return tw.get(s0 + t, g); });
        for (int t = 0; t < 4; t++)
        {
            stage_by_bit(y, m, tw, s0 + t);
            if (t + 1 == FIXAT)
                fix_all(y, m);
        }
    }
    // the phase templates against the same stages run one at a time (checked after every stage), bit for bit
    SHL_HD void compare_phase(const double (&x)[16], const double (&y)[16], const FpDesc &m, Sink &sk, uint64_t tag)
    {
        for (int a = 0; a < 16; a++)
        {
            sk.out(x[a]);
            FPC_EXPECT(fp_to_bits(x[a]) == fp_to_bits(y[a]), 24u, fp_to_bits(x[a]), tag);
        }
    }
    SHL_HD void seed_inputs(double (&x)[16], uint64_t (&ref)[16], double mag, uint64_t v, const FpDesc &m)
    {
        for (int a = 0; a < 16; a++)
        {
            x[a] = (v >> a) & 1 ? -mag : mag;
            ref[a] = canon(x[a], m.qi);
        }
    }
    SHL_HD void phase_cases(const FpDesc &m, const TwSet &tw, Rng &rng, unsigned it, Sink &sk)
    {
        const uint64_t q = m.qi;
        const double half = (double)(q / 2);
        // a four-stage phase: phase_fwd_end<true, 4, true> and phase_fwd_fix<true, 4, FIXAT>
        {
            double x[16], y[16], z[16];
            uint64_t ref[16], rz[16];
            const uint64_t v = (it & 3) == 0 ? 0 : rng.next();
            seed_inputs(x, ref, half, v, m);
            for (int a = 0; a < 16; a++)
                y[a] = z[a] = x[a], rz[a] = ref[a];
            phase_fwd_end<true, 4, true>(x, m, [&](int t, int g) { return tw.get(t, g); });
            for (int t = 0; t < 4; t++)
            {
                stage_by_bit(y, m, tw, t);
                ref_stage_fwd(ref, 3 - t, tw, t, q);
                check_regs(y, ref, ladder(0.5, t + 1), m, sk, 20u, 21u, 22u, 0x100u + t);
            }
            fix_all(y, m);
            compare_phase(x, y, m, sk, 0x10);
            check_regs(x, ref, 0.5, m, sk, 25u, 21u, 22u, 0x10);
            for (int a = 0; a < 16; a++)
                y[a] = z[a];
            switch (it % 3)
            {
            case 0: phase_fix_case<1>(z, y, m, tw, 4); break;
            case 1: phase_fix_case<2>(z, y, m, tw, 4); break;
            default: phase_fix_case<3>(z, y, m, tw, 4); break;
            }
            for (int t = 0; t < 4; t++)
                ref_stage_fwd(rz, 3 - t, tw, 4 + t, q);
            compare_phase(z, y, m, sk, 0x20 + it % 3);
            check_regs(z, rz, ladder(0.5, 3 - (int)(it % 3)), m, sk, 25u, 21u, 22u, 0x20 + it % 3);
        }
        // the lean sixteen stages of the key switch (p1_tile / p2_tile with LEAN): four stages, phase_fwd_fix<.., FPC_LEAN_FIX1>,
        // the crossing through the packed words, four stages, phase_fwd_fix<.., 1>; the digit enters fixed or at kLeanEntryQ q
        {
            const double entry_q = (it & 1) ? kLeanEntryQ : 0.5;
            double x[16], y[16];
            uint64_t ref[16];
            seed_inputs(x, ref, units(entry_q, m), (it & 2) ? rng.next() : 0, m);
            for (int a = 0; a < 16; a++)
                y[a] = x[a];
            double bq = entry_q;
            int s = 0;
            auto staged = [&](int nst, int fixat) {
                for (int t = 0; t < nst; t++, s++)
                {
                    stage_by_bit(y, m, tw, s);
                    ref_stage_fwd(ref, 3 - (s & 3), tw, s, q);
                    bq = ladder(bq, 1);
                    FPC_EXPECT(bq * m.q + 2.0 < kTwo53, 23u, (uint64_t)s, fp_to_bits(bq));
                    check_regs(y, ref, bq, m, sk, 20u, 21u, 22u, 0x200u + s);
                    if (t + 1 == fixat)
                    {
                        fix_all(y, m);
                        bq = 0.5;
                    }
                }
            };
            phase_fwd_end<true, 4, false>(x, m, [&](int t, int g) { return tw.get(t, g); });
            staged(4, 0);
            compare_phase(x, y, m, sk, 0x30);
            phase_fwd_fix<true, 4, FPC_LEAN_FIX1>(x, m, [&](int t, int g) { return tw.get(4 + t, g); });
            staged(4, FPC_LEAN_FIX1);
            compare_phase(x, y, m, sk, 0x31);
            // the crossing: below 2^51 and at most 1.80 q, and the packed words give the same doubles back
            double cross = 0.0;
            for (int a = 0; a < 16; a++)
                cross = fabs_(x[a]) > cross ? fabs_(x[a]) : cross;
            sk.mag(kSlotCross, cross / m.q);
            FPC_EXPECT(cross < kTwo51, 26u, fp_to_bits(cross), it);
            FPC_EXPECT(cross <= 1.80 * m.q + 2.0, 27u, fp_to_bits(cross), it);
            uint64_t w[13];
            double u[16];
            pack52(x, w);
            unpack52(w, u);
            for (int a = 0; a < 16; a++)
                FPC_EXPECT(fp_to_bits(u[a]) == fp_to_bits(x[a]), 40u, fp_to_bits(x[a]), a);
            for (int a = 0; a < 16; a++)
                x[a] = u[a];
            phase_fwd_end<true, 4, false>(x, m, [&](int t, int g) { return tw.get(8 + t, g); });
            staged(4, 0);
            compare_phase(x, y, m, sk, 0x32);
            phase_fwd_fix<true, 4, 1>(x, m, [&](int t, int g) { return tw.get(12 + t, g); });
            staged(4, 1);
            compare_phase(x, y, m, sk, 0x33);
            const double mx = check_regs(x, ref, 2.64, m, sk, 25u, 21u, 22u, 0x33);
            sk.mag(kSlotLeanOut, mx / m.q);
        }
    }

    // inverse: phase_inv<true, 4, 0>, and phase_inv<true, 4, 1> + inv_last_stage<true, ...>
    SHL_HD void inverse_cases(const FpDesc &m, const TwSet &tw, Rng &rng, unsigned it, Sink &sk)
    {
        const uint64_t q = m.qi;
        const double half = (double)(q / 2), qd = m.q;
        double x[16], z[16];
        uint64_t ref[16], rz[16];
        seed_inputs(x, ref, half, (it & 1) ? rng.next() : ((it & 2) ? 0xAAAAull : 0), m);
        for (int a = 0; a < 16; a++)
            z[a] = x[a], rz[a] = ref[a];
        phase_inv<true, 4, 0>(x, m, [&](int t, int g) { return tw.get(t, g); });
        for (int t = 3; t >= 0; t--)
            ref_stage_inv(ref, 3 - t, tw, t, q);
        // sums double per stage (0.5 -> 8 q at the most, exact), a product of a difference below 2 B q is below q (0.5 + 0.375 B)
        for (int a = 0; a < 16; a++)
        {
            sk.out(x[a]);
            FPC_EXPECT(is_int53(x[a]) && canon(x[a], q) == ref[a], 30u, fp_to_bits(x[a]), a);
            FPC_EXPECT(fabs_(x[a]) <= 8.0 * qd, 31u, fp_to_bits(x[a]), a);
            sk.mag(kSlotInv + 4, fabs_(x[a]) / qd);
        }
        // three stages, then the last one with N^-1 folded in: X' = (X + Y) ni, Y' = (X - Y) nw
        phase_inv<true, 4, 1>(z, m, [&](int t, int g) { return tw.get(t, g); });
        for (int t = 3; t >= 1; t--)
            ref_stage_inv(rz, 3 - t, tw, t, q);
        double smax = 0.0;
        for (int k = 0; k < 8; k++)
        {
            const double s = fabs_(z[k] + z[k | 8]), d = fabs_(z[k] - z[k | 8]);
            smax = s > smax ? s : smax;
            smax = d > smax ? d : smax;
        }
        sk.mag(kSlotInv + 3, smax / (2.0 * qd));
        const double ni = tw.lane[it & 15], nw = tw.get(0, 0);
        inv_last_stage<true, 4, 2, 0>(z, m, ni, nw);
        const uint64_t nic = canon(ni, q), nwc = canon(nw, q);
        for (int k = 0; k < 8; k++)
        {
            const uint64_t a = rz[k], b = rz[k | 8];
            rz[k] = mulq(addq(a, b, q), nic, q);
            rz[k | 8] = mulq(subq(a, b, q), nwc, q);
        }
        for (int a = 0; a < 16; a++)
        {
            sk.out(z[a]);
            FPC_EXPECT(is_int53(z[a]) && canon(z[a], q) == rz[a], 32u, fp_to_bits(z[a]), a);
            FPC_EXPECT(smax < kTwo53 && fabs_(z[a]) <= qd * (0.5 + 0.1875 * smax / qd) + 2.0, 33u, fp_to_bits(z[a]), fp_to_bits(smax));
            sk.mag(kSlotInvLast, fabs_(z[a]) / qd);
        }
    }

    // ---- the packed intermediate
    SHL_HD void pack_cases(const FpDesc &m, Rng &rng, unsigned it, Sink &sk)
    {
        const double e = units(1.80, m);
        const double fixed[9] = { 0.0, 1.0, -1.0, kTwo51 - 1.0, -(kTwo51 - 1.0), -kTwo51, e, -e, e - 1.0 };
        double x[16], u[16];
        uint64_t w[13];
        for (int a = 0; a < 16; a++)
        {
            const int slot = (a + (int)it) & 15; // every value visits every slot
            const uint64_t v = rng.next();
            x[slot] = a < 9 ? fixed[a] : (double)((int64_t)(v >> 12) - (int64_t)(1ull << 51));
        }
        pack52(x, w);
        unpack52(w, u);
        for (int k = 0; k < 13; k++)
            sk.word(w[k]);
        for (int a = 0; a < 16; a++)
            FPC_EXPECT(fp_to_bits(u[a]) == fp_to_bits(x[a] + 0.0), 40u, fp_to_bits(x[a]), a);
    }

    // ---- the key switch's accumulator: RUN terms between two acc_fix, up to kMaxKeyComps terms
    template <int RUN, bool ASSERT>
    SHL_HD void acc_case(const FpDesc &m, Rng &rng, unsigned it, int slot, Sink &sk)
    {
        typedef Field<true> F;
        const uint64_t q = m.qi, h = q / 2;
        const double qd = m.q, xm = units(2.64, m), term_q = 0.5 + 0.1875 * 2.64; // 0.995
        F::Acc a = F::acc_zero();
        uint64_t ref = 0;
        double bound = 0.0; // of |a|: q / 2 + 3 after a fix (fp_fix above, |a| < 2^53), + 0.995 q + 2 per term
        for (unsigned j = 0; j < kMaxKeyComps; j++)
        {
            const uint64_t v = rng.next();
            const double xa = (v & 1) ? xm : (double)(int64_t)((v >> 11) % ((uint64_t)xm + 1));
            uint64_t ka;
            switch ((v >> 1) & 3)
            {
            case 0: ka = h - ((v >> 3) & 3); break;
            case 1: ka = 1 + ((v >> 3) & 15) % h; break;
            case 2:
            {
                // a key word that puts x k next to (k' + 1/2) q
                const uint64_t xi = (uint64_t)xa ? (uint64_t)xa : 1, kmax = udiv128((u128)h * xi, q);
                ka = tie_point(kmax ? (v >> 8) % kmax : 0, q, xi);
                ka = ka > h ? h : ka;
                break;
            }
            default: ka = (v >> 8) % (h + 1); break;
            }
            const double k = (v >> 7) & 1 ? -(double)ka : (double)ka;
            // the sign of x that makes the term add to the running sum
            const double probe = fp_mulmod(xa, k, m.q, m.qinv);
            const double x = ((probe < 0.0) != (a < 0.0)) ? -xa : xa;
            F::mac(a, x, k, m);
            sk.out(a);
            ref = addq(ref, mulq(canon(x, q), canon(k, q), q), q);
            bound += term_q * qd + 2.0;
            if (ASSERT)
            {
                FPC_EXPECT(bound < kTwo53, 53u, j, fp_to_bits(bound));
                FPC_EXPECT(fabs_(a) < kTwo53, 50u, fp_to_bits(a), j);
                FPC_EXPECT(is_int53(a) && canon(a, q) == ref && fabs_(a) <= bound, 51u, fp_to_bits(a), j);
            }
            if (fabs_(a) < kTwo53)
                sk.mag(slot, fabs_(a) / qd);
            if (j % RUN == RUN - 1)
            {
                F::acc_fix(a, m);
                sk.out(a);
                bound = 0.5 * qd + 3.0;
            }
            if (ASSERT && (j == 0 || j == kMaxKeyComps - 1 || (j & 7) == (it & 7)))
            {
                const uint64_t c = F::acc_to_canon(a, m);
                sk.word(c);
                FPC_EXPECT(c == ref, 52u, fp_to_bits(a), j);
            }
        }
    }

    // one (prime, thread, round).  `block` = the thread's workgroup: what the wave-uniform twiddle index is made of.
    SHL_HD void run_round(const FpDesc &m, const double *utab, unsigned prime, unsigned block, unsigned thread, unsigned round, Sink &sk)
    {
        Rng rng{ seed_of(prime, thread, round) };
        rng.next();
        TwSet tw;
        tw.utab = utab;
        tw.ub = block * 7u + round * 13u;
        fill_lane_tw(tw, m, rng);
        prim_cases(m, rng, round + thread, sk);
        use_site_cases(m, rng, round + thread, sk);
        staged_growth<false>(m, tw, rng, 0.5, 7, sk);
        staged_growth<true>(m, tw, rng, 0.5, 7, sk);
        staged_growth<true>(m, tw, rng, kLeanEntryQ, 4 + FPC_LEAN_FIX1, sk); // an unfixed digit up to the lean run's first fix
        phase_cases(m, tw, rng, round + thread, sk);
        inverse_cases(m, tw, rng, round + thread, sk);
        pack_cases(m, rng, round + thread, sk);
        acc_case<FPC_ACC_RUN, true>(m, rng, round + thread, kSlotAcc, sk);
        if (FPC_ACC_RUN != 8 && ((round + thread) & 3) == 0)
            acc_case<8, false>(m, rng, round + thread, kSlotAcc8, sk);
    }

    // ---- reporting (host side of either program)
    inline const char *slot_name(int s)
    {
        static const char *names[kMaxSlots] = { "", "fwd stage 1", "fwd stage 2", "fwd stage 3", "fwd stage 4", "fwd stage 5", "fwd stage 6", "fwd stage 7",
                                                "crossing", "lean exit", "", "", "inv sums (3 stages, /2q)", "inv phase out", "inv last stage",
                                                "acc, fix every 7", "acc, fix every 8", "", "", "", "", "", "", "" };
        return names[s];
    }
    // The streams both programs run, and whose doubles the digest covers: workgroups [0, kDigestBlocks) of kThreadsPerBlock
    // threads, rounds [0, kDigestRounds).  The device check runs more workgroups and more rounds on top of them (checked, not
    // folded); the host's share is sized by what tests/test_emu_parity.py::test_field_arithmetic_exact may take.
    constexpr unsigned kThreadsPerBlock = 256, kDigestBlocks = 4, kDigestRounds = 4;
    // prints the per-prime lines and the digest line; returns the number of failures
    inline unsigned long long report(const char *prog, const Result *res, unsigned long long *digest_out = nullptr)
    {
        unsigned long long fails = 0, digest = 0, code = 0;
        Result all{};
        for (unsigned p = 0; p < kNumPrimes; p++)
        {
            const Result &r = res[p];
            fails += r.fails;
            code = r.code > code ? r.code : code;
            digest += r.digest * (2 * p + 1);
            if (r.fails)
                std::printf("%s: q=%llu: %llu failures, highest failing check %llu; first: check %llu q=%llu operands 0x%016llx 0x%016llx\n", prog, (unsigned long long)primes()[p],
                            r.fails, r.code, r.first[0], r.first[1], r.first[2], r.first[3]);
            std::printf("%s: q=%llu max |x|/q:", prog, (unsigned long long)primes()[p]);
            for (int s = 1; s < kMaxSlots; s++)
                if (slot_name(s)[0])
                {
                    std::printf(" %s%.4f", s == 1 ? "fwd 1..7 " : s <= 7 ? "" : (std::string(slot_name(s)) + " ").c_str(), fp_from_bits(r.maxq[s]));
                    all.maxq[s] = r.maxq[s] > all.maxq[s] ? r.maxq[s] : all.maxq[s];
                }
            std::printf("\n");
        }
        std::printf("%s: all primes, max |x|/q:", prog);
        for (int s = 1; s < kMaxSlots; s++)
            if (slot_name(s)[0])
                std::printf(" [%s] %.4f", slot_name(s), fp_from_bits(all.maxq[s]));
        std::printf("\n%s digest %016llx\n", prog, digest);
        if (fails)
            std::printf("%s: %llu failures, highest failing check %llu\n", prog, fails, code);
        if (digest_out)
            *digest_out = digest;
        return fails;
    }
} // namespace fpcases
