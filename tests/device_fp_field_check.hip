// Device-side check of the double-precision back end (field.h, Field<true>) and of the phase templates of ntt2_device.h that place
// its range reductions, at the bounds field.h documents: the case body of tests/fp_field_cases.h - the same source the host check
// tests/field_check.cpp runs serially - compiled for gfx950 with the library's own flags, every thread drawing its own operands
// and comparing with 128-bit integer arithmetic.  The per-prime constants arrive through ld_uniform_fpd, the twiddles alternately
// through ld_uniform(const double *, idx) and from per-lane registers.  The kernel's only stores are atomics on its result buffer
// (one Result per prime); the operands live in registers.  Prints the digest of the streams it shares with the host check.
// Test infrastructure: built by seal_amd/csrc/Makefile (target devcheck) into seal_amd/lib/, run by
// tests/test_gpu_parity.py::test_device_fp_field_check.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fp_field_cases.h"

using namespace fpcases;

constexpr unsigned kBlocks = 64, kRounds = 12; // workgroups per prime, rounds per thread (the digest's share: fp_field_cases.h)
static_assert(kBlocks >= kDigestBlocks && kRounds >= kDigestRounds, "the device runs the host's streams and more");

__global__ void __launch_bounds__(kThreadsPerBlock) fp_check_kernel(const FpDesc *fpd, const double *utab, unsigned rounds, Result *res)
{
    const unsigned p = blockIdx.y;
    const FpDesc m = ld_uniform_fpd(&fpd[p]);
    const unsigned thread = blockIdx.x * kThreadsPerBlock + threadIdx.x;
    Sink shared = sink_zero(true), extra = sink_zero(false);
    for (unsigned r = 0; r < rounds; r++)
    {
        const bool in_digest = blockIdx.x < kDigestBlocks && r < kDigestRounds;
        run_round(m, utab + p * kUniTw, p, blockIdx.x, thread, r, in_digest ? shared : extra);
    }
    merge(res[p], shared);
    merge(res[p], extra);
}

int main()
{
    std::vector<FpDesc> fpd;
    std::vector<double> utab(kNumPrimes * kUniTw);
    for (unsigned p = 0; p < kNumPrimes; p++)
    {
        fpd.push_back(make_desc(primes()[p]));
        fill_uniform_tw(primes()[p], p, utab.data() + p * kUniTw);
    }
    FpDesc *dm;
    double *dt;
    Result *dr;
    if (hipMalloc(&dm, fpd.size() * sizeof(FpDesc)) != hipSuccess || hipMalloc(&dt, utab.size() * sizeof(double)) != hipSuccess ||
        hipMalloc(&dr, kNumPrimes * sizeof(Result)) != hipSuccess)
    {
        printf("device_fp_field_check: no device memory\n");
        return 2;
    }
    (void)hipMemcpy(dm, fpd.data(), fpd.size() * sizeof(FpDesc), hipMemcpyHostToDevice);
    (void)hipMemcpy(dt, utab.data(), utab.size() * sizeof(double), hipMemcpyHostToDevice);
    (void)hipMemset(dr, 0, kNumPrimes * sizeof(Result));
    hipLaunchKernelGGL(fp_check_kernel, dim3(kBlocks, kNumPrimes), dim3(kThreadsPerBlock), 0, 0, dm, dt, kRounds, dr);
    std::vector<Result> res(kNumPrimes);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(res.data(), dr, kNumPrimes * sizeof(Result), hipMemcpyDeviceToHost) != hipSuccess)
    {
        printf("device_fp_field_check: kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    if (report("device_fp_field_check", res.data()))
        return 1;
    printf("device_fp_field_check ok (%u primes x %u threads x %u rounds)\n", kNumPrimes, kBlocks * kThreadsPerBlock, kRounds);
    return 0;
}
