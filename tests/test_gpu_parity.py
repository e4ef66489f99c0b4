"""GPU (MI355X) parity tests — the tests proper.  Everything goes through the C ABI of the gfx950 build
(seal_amd/lib/libsealhip.so); outputs are compared bit-for-bit with the oracle (the real reference when
oracle/_ref travelled with the repo, else the plain-C restatement) on identical inputs and key words,
at test sizes, at the BASELINE.json configurations, and against the committed golden vectors."""
import os

import numpy as np
import pytest

import parity_cases as P
import sealref as R
from harness import DeviceSide
from oracle import Oracle, coeff_modulus_create, kind_available, plain_modulus_batching, rand_ct

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_native_library_is_the_one_loaded(gpu):
    """The HIP extension must be what runs: in-tree .so, real device, no fallback."""
    from seal_amd import _native
    assert _native._lib_path.endswith(os.path.join("seal_amd", "lib", "libsealhip.so"))
    name, cus, mem = gpu.device_info()
    assert cus >= 64 and mem > (64 << 30)
    with open("/proc/self/maps") as f:
        assert any("libsealhip.so" in line for line in f)


# ---- NTT at every plan, incl. BASELINE config 2 (CKKS N=8192, L=4: fwd + inv over all components)
@pytest.mark.parametrize("n,bits,polys", [
    (2, [30, 30], 2), (16, [30, 30], 3), (64, [40, 50], 3), (128, [40, 50], 2), (256, [50, 60], 2), (512, [50], 5),
    (1024, [50, 60], 2), (2048, [60], 3), (4096, [36, 36, 37], 4),
    (8192, [60, 40, 40, 60], 6),            # BASELINE configs[1]
    (16384, [60, 50, 50], 3), (32768, [55, 55], 2), (65536, [60, 50, 60], 2), (131072, [60], 1),
    # integer back end, unguarded butterflies: user moduli of 51 .. 60 bits in the two-pass engine
    (8192, [60, 59, 58], 5), (16384, [58, 60], 3), (32768, [60, 55, 52], 2), (65536, [60, 59, 51], 2),
])
def test_ntt(gpu, n, bits, polys):
    P.case_ntt(n, bits, polys=polys)


def test_ntt_more_polynomials_than_one_grid(gpu):
    """66000 polynomials at N = 8: the launcher's loop over grids of 65535 outer items takes its second iteration.  (The two-pass
    engine has the same loop; reaching it needs 4 GB per component and is left out.)"""
    P.case_ntt_many_polys()


# single-launch transforms (N = 2^13, 2^14): batches large enough that every workgroup loops with the next
# transform in flight, and a forced one-workgroup-per-component loop
@pytest.mark.parametrize("n,bits,polys,chunks", [
    (8192, [50, 36, 60], 5, 2), (8192, [50, 40, 40], 1100, 0), (16384, [50, 45, 60], 3, 1), (16384, [50, 50], 600, 0),
    # integer back end in one launch (round 3), the three modulus classes; BASELINE configs[1]'s own chain at a bench-sized batch
    (8192, [60, 59, 57, 55], 5, 2), (8192, [60, 40, 40, 60], 600, 0), (16384, [58, 60, 51], 3, 1), (16384, [59, 57], 300, 0),
])
def test_ntt_single_launch_loop(gpu, monkeypatch, n, bits, polys, chunks):
    if chunks:
        monkeypatch.setenv("SEALHIP_NTT_FCHUNKS", str(chunks))
    P.case_ntt(n, bits, polys=polys)


# two-pass engine at N = 2^15 / 2^16 with batches large enough that every workgroup LOOPS over its share (next tile in flight,
# pass 2's twiddles hoisted: ntt2_fwd_p2<D1, 4>) - the shape of bench.py's roofline leg, which no other test compares with the
# reference - and, at 2^16, the packed intermediate of the double-precision components (ntt2_kernels.hip: kPackWords)
@pytest.mark.parametrize("n,bits,polys", [(65536, [50, 40, 60], 400), (65536, [45, 50], 700), (32768, [50, 60, 50], 500)])
def test_ntt_two_pass_loop(gpu, n, bits, polys):
    P.case_ntt(n, bits, polys=polys)


# the ONE-launch kernel of N = 2^16 (ntt2_ring.hip: both passes in every workgroup, the intermediate in a re-used ring, hand-over by
# progress words) - opt-in (SEALHIP_NTT_RING=1, read once per process, hence the child), every polynomial against the reference;
# ragged slices (301 = 16 teams x 18 or 19 iterations), one and three double-precision components next to integer ones
@pytest.mark.parametrize("mode", [1, 2])   # 1: every workgroup does both passes; 2: pass-1 and pass-2 workgroups side by side
@pytest.mark.parametrize("bits,polys", [([50, 45, 60, 50], 301), ([45, 60], 700), ([50] * 8, 160)])
def test_ntt_ring_one_launch(gpu, bits, polys, mode):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import parity_cases as P; P.case_ntt(65536, %r, polys=%d)" % (here, bits, polys)
    env = dict(os.environ, SEALHIP_NTT_RING=str(mode), SEALHIP_RING_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ran = [line for line in r.stderr.splitlines() if line.startswith("ntt2_fwd_ring:")]
    assert ran, "the ring kernel did not run: " + r.stderr[-2000:]
    assert all(" lost 0," in line for line in ran), ran


# ---- structured worst-case inputs at every engine plan: all q-1, all 0, alternating, floor(q/2), floor(q/2)+1, a
#      spike at N-1, a random mix of those, all ones - one prime below 2^50, one 60-bit, one of 51 .. 59 bits
@pytest.mark.parametrize("n,bits,polys", [
    (4096, [36, 60, 55], 8), (8192, [50, 60, 58], 8), (16384, [45, 60, 51], 8), (32768, [50, 60, 55], 8), (65536, [50, 60, 59], 8),
    (8192, [50, 60, 58], 1104),      # single-launch kernels, looping workgroups
    (65536, [49, 60, 57], 400),      # two-pass engine, looping workgroups, packed intermediate
])
def test_extremes_ntt(gpu, n, bits, polys):
    P.case_extremes_ntt(n, bits, polys)


@pytest.mark.parametrize("n,bits,batch,check", [
    (4096, [50, 36, 36, 50], 8, None), (8192, [60, 40, 58, 60], 8, None), (16384, [60, 50, 55, 60], 8, None),
    (65536, [60, 50, 49, 57, 60], 8, None),
    (65536, [60] + [50] * 14 + [60], 64, (0, 1, 2, 3, 4, 5, 6, 7, 33, 63)),   # BASELINE configs[4] / the headline chain, chunked key switch
])
def test_extremes_ckks(gpu, n, bits, batch, check):
    P.case_extremes_ckks(n, bits, batch=batch, check=check)


@pytest.mark.parametrize("n,bits", [(4096, [36, 36, 37]), (8192, [50, 55, 60]), (16384, [55, 55, 55, 55])])
def test_extremes_bfv(gpu, n, bits):
    primes = coeff_modulus_create(n, bits)
    P.case_extremes_bfv(n, primes, plain_modulus_batching(n, 20))


# deferred tensor products (evaluator.h: LazyProduct): the fused multiply -> relinearize and the life cycle of a pending product, at
# every two-pass size, small batches through the test knobs and - the third case - the batch the launcher defers by its own rule
@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 3), (16384, [60, 50, 55, 50, 60], 2), (32768, [50, 59, 50, 60], 2),
                                          (65536, [60, 50, 50, 49, 60], 5)])
def test_lazy_product_life_cycle(gpu, n, bits, batch):
    P.case_lazy_product(n, bits, batch=batch)


# rotations without the permutation kernels (round 6): every two-pass size, small batches through SEALHIP_KS_SPLIT=1 and - the last
# case - a batch the launcher takes there by its own rule (chunked key switch on lanes at 2^16)
@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 3), (16384, [60, 50, 55, 50, 60], 2), (32768, [50, 59, 50, 60], 2),
                                          (65536, [60, 50, 50, 49, 60], 5), (65536, [60, 50, 50, 60], 70)])
def test_rotate_gather(gpu, n, bits, batch):
    P.case_rotate_gather(n, bits, batch=batch, steps=(1, -1) if batch < 10 else (1,))


def test_pending_product_threads(gpu):
    """two host threads around pending tensor products (one destination read by both: formed once; one operand shared by two fused
    relinearisations on two evaluators / streams)"""
    P.case_pending_product_threads(8192, (50, 40, 40, 60), rounds=8)
    P.case_pending_product_threads(65536, (60, 50, 50, 60), rounds=3)


def test_dyadic(gpu):
    P.case_dyadic(4096, [60, 40, 30])


def test_kats_on_device(gpu):
    """native/tests/seal/util/ntt.cpp:75-101 and galois.cpp:86-120 through the GPU path."""
    S = gpu
    d = DeviceSide("ckks", 2, [0xFFFFFFFFFFC0001])
    assert d.ctx.ntt_root(0) == 288794978602139552
    buf = S.DeviceBuffer.from_numpy(np.array([1, 1], dtype=np.uint64))
    S.ntt_forward(d.ctx, buf, 1, 1)
    assert list(buf.to_numpy((2,))) == [288794978602139553, 864126526004445282]
    d = DeviceSide("ckks", 8, [17])
    src = S.DeviceBuffer.from_numpy(np.arange(8, dtype=np.uint64))
    dst = S.DeviceBuffer(8)
    S.apply_galois(d.ctx, 0, False, 3, src, dst, 1)
    assert list(dst.to_numpy((8,))) == [0, 14, 6, 1, 13, 7, 2, 12]
    S.apply_galois(d.ctx, 0, True, 3, src, dst, 1)
    assert list(dst.to_numpy((8,))) == [4, 5, 7, 6, 1, 0, 2, 3]


# ---- CKKS pipelines: small, ragged batch, and BASELINE configs 3 and 5
@pytest.mark.parametrize("n,bits,batch,steps", [
    (16, [30, 30, 30, 30], 3, (1, -1)),
    (1024, [50, 40, 40, 50], 5, (1,)),
    (8192, [60, 40, 40, 60], 2, (1, 7)),
    (16384, [60, 50, 50, 50, 50, 50, 50, 60], 2, (1,)),                 # BASELINE configs[2]
])
def test_ckks_pipeline(gpu, n, bits, batch, steps):
    P.case_ckks_pipeline(n, bits, batch=batch, steps=steps)


@pytest.mark.parametrize("n,bits", [
    (8192, [60] + [30, 40, 50, 45, 36] * 4 + [60]),           # 22 primes, mixed sizes: 21 digits, both arithmetic classes interleaved
    (16384, [60] + [50, 40, 48, 36, 44, 58] * 5 + [60]),      # 32 primes incl. 58-bit ones: 31 digits (sums fixed every 8 terms, 4 times)
    (65536, [55] + [45, 50] * 9 + [59]),                      # N = 2^16 with the lean placement on unequal prime sizes, 20 primes
])
def test_ckks_long_mixed_chains(gpu, n, bits):
    """long coefficient-modulus chains with unequal prime sizes: digits from larger primes raised to smaller target moduli, many
    terms per key-switch sum, integer and double-precision targets interleaved (evaluator.cpp:2561-2867)"""
    P.case_ckks_pipeline(n, bits, batch=1, steps=(1,), check_transforms=n <= 16384)


def test_ckks_north_star_config(gpu):
    """BASELINE configs[4] / north-star: CKKS N=65536, L=16 ({60, 14x50, 60}): multiply + relinearize +
    rescale_to_next, then rotate_vector(1) + mod_switch, batch of 2, bit-exact."""
    P.case_ckks_pipeline(65536, [60] + [50] * 14 + [60], batch=2, steps=(1,), check_transforms=False)


# ---- parity at the launch configuration bench.py times: un-split key switch, many items per (I, tile)
def test_ckks_north_star_unsplit_key_switch(gpu, monkeypatch):
    """C5 with SEALHIP_KS_SPLIT=1: the one-group-per-workgroup ks1/ks2 kernels that batch >= 8 selects (bench.py: batch 256),
    here forced at batch 2; multiply + relinearize + rescale + rotate item by item vs the reference."""
    monkeypatch.setenv("SEALHIP_KS_SPLIT", "1")
    P.case_ckks_pipeline(65536, [60] + [50] * 14 + [60], batch=2, steps=(1,), check_transforms=False)


def test_ckks_north_star_batch16(gpu):
    """C5, batch 16: split = 1 by the launcher's own rule, XCD-ordered grid over several batch items per (I, tile);
    every item of every stage compared with the reference (evaluator.cpp:2561-2867)."""
    P.case_ckks_pipeline(65536, [60] + [50] * 14 + [60], batch=16, steps=(1,), check_transforms=False)


def test_ckks_batch1024_scratch_beyond_2_pow_32_words(gpu):
    """batch 1024 at a two-pass size (CKKS N=32768, K=13): the key-switch intermediate is 1024*14*13*32768 = 6.1e9 words,
    beyond 2^32 — index arithmetic of the batched launches; sampled items vs the reference."""
    P.case_ckks_big_batch(32768, [60] + [50] * 12 + [60], batch=1024, check_items=(0, 1, 511, 512, 777, 1023))


def test_ckks_north_star_batch256_sampled(gpu):
    """the shape bench.py times (C5, batch 256, intermediate 4.03e9 words): first / middle / last items vs the reference"""
    P.case_ckks_big_batch(65536, [60] + [50] * 14 + [60], batch=256, check_items=(0, 127, 128, 255))


def test_ckks_north_star_batch512_bounded_scratch(gpu, monkeypatch):
    """VERDICT r4 missing #4: the key switch's intermediate (126 MB per C5 ciphertext) is bounded by chunking the batch
    (sealhip.h: Chunked key switching).  C5 at batch 512 with a 4 GiB cap: the whole batch would need 64.5 GB, the chunks hold at
    most the cap; items of the first, a middle and the last chunk (and the ragged edges between chunks) vs the reference
    (evaluator.cpp:2561-2867 holds O(K N) per ciphertext)."""
    import seal_amd as S
    monkeypatch.setenv("SEALHIP_KS_SCRATCH_CAP_MIB", "4096")
    c0, k0, _ = S.ks_chunk_stats()
    P.case_ckks_big_batch(65536, [60] + [50] * 14 + [60], batch=512, check_items=(0, 15, 16, 255, 256, 300, 511), unique=64)
    c1, k1, held = S.ks_chunk_stats()
    assert c1 - c0 == 2, "relinearize and rotate_vector both run in chunks"
    assert k1 - k0 >= 2 * 4 * 4, ("at least 16 chunks per key switch under a 4 GiB cap", k1 - k0)
    assert held <= 4096 * 1048576, held


def test_ks_chunked_lanes(gpu):
    """the chunked key switch at a small two-pass size on real streams: 3 lanes, ragged last chunk, CKKS folded tail and BFV
    (the target read in place), each against the unchunked run and the reference"""
    P.case_ks_chunked("ckks", 8192, [50, 40, 40, 50], batch=11, chunk=3, lanes=3)
    P.case_ks_chunked("ckks", 16384, [60, 50, 50, 50, 60], batch=9, chunk=2, lanes=4)
    pr = coeff_modulus_create(8192, [45, 40, 45])
    P.case_ks_chunked("bfv", 8192, pr, batch=6, chunk=2, lanes=2, t=plain_modulus_batching(8192, 20))


# ---- BFV pipelines: small, BASELINE config 1 (N=4096 BFVDefault sizes) and config 4 (N=32768, 14 primes)
@pytest.mark.parametrize("n,bits,tb,batch", [
    (16, [30, 30, 30, 30], 12, 3),
    (4096, [36, 36, 37], 20, 2),            # BASELINE configs[0]
    (8192, [55] * 5, 20, 1),
])
def test_bfv_pipeline(gpu, n, bits, tb, batch):
    primes, t = P.default_bfv_params(n, bits, tb)
    P.case_bfv_pipeline(n, primes, t, batch=batch)


def test_bfv_config4(gpu):
    """BASELINE configs[3]: BFV N=32768, 14x55-bit chain, Batching(32768, 20): multiply + relinearize +
    mod_switch (one ciphertext here; the 1024-ciphertext sharding is bench.py's job)."""
    primes, t = P.default_bfv_params(32768, [55] * 14, 20)
    P.case_bfv_pipeline(32768, primes, t, batch=1)


# ---- BGV pipelines (SURVEY §8a E2, E6 BGV branch, E8 BGV branch): small, single-pass and two-pass engine sizes
@pytest.mark.parametrize("n,bits,tb,batch", [
    (16, [30, 30, 30, 30], 12, 3),
    (4096, [36, 36, 37], 20, 2),
    (8192, [50, 55, 56, 60], 20, 2),
    (32768, [55] * 6, 20, 1),
])
def test_bgv_pipeline(gpu, n, bits, tb, batch):
    if not R.available():
        pytest.skip("BGV parity needs the real reference (oracle/_ref)")
    primes, t = P.default_bfv_params(n, bits, tb)
    P.case_bgv_pipeline(n, primes, t, batch=batch)


# ---- digit-parallel key switching (sealhip.h section 1b; BASELINE configs[4]), ranks emulated in one process
@pytest.mark.parametrize("scheme,n,bits,tb,parts,batch", [
    ("ckks", 1024, [50, 40, 40, 50], 0, 2, 2),
    ("ckks", 8192, [60, 40, 40, 50, 60], 0, 3, 2),
    ("bfv", 8192, [55] * 4, 20, 2, 1),
    ("bgv", 8192, [55] * 4, 20, 3, 1),
    ("ckks", 65536, [60] + [50] * 14 + [60], 0, 8, 1),      # north-star parameters, 15 digits over 8 ranks
])
def test_digit_parallel_key_switch(gpu, scheme, n, bits, tb, parts, batch):
    if scheme == "bgv" and not R.available():
        pytest.skip("BGV parity needs the real reference (oracle/_ref)")
    primes = coeff_modulus_create(n, bits)
    t = plain_modulus_batching(n, tb) if tb else 0
    P.case_digit_parallel(scheme, n, primes, t, parts=parts, batch=batch)


@pytest.mark.parametrize("n,bits,parts,batch", [
    (1024, [50, 40, 40, 50], 4, 2),
    (8192, [60, 40, 40, 50, 60], 3, 2),
    (65536, [60] + [50] * 14 + [60], 8, 1),      # north-star parameters: 15 digits / 15 moduli over 8 ranks
])
def test_digit_parallel_reduce_scatter(gpu, n, bits, parts, batch):
    """exchange 1 of sealhip.h section 1c (reduce-scatter by target modulus + all-gather): emulated ranks on one GPU, then the
    library's own driver and key broadcast through a ONE-RANK RCCL communicator (real ncclReduceScatter / AllGather /
    AllReduce / Broadcast calls on the evaluator's stream)"""
    import seal_amd as S
    primes = coeff_modulus_create(n, bits)
    loopback = P.case_digit_parallel_reduce_scatter(n, primes, parts=parts, batch=batch)
    assert S.Comm.rccl_available(), "librccl.so.1 did not load on the GPU box"
    assert loopback is False, "the communicator fell back to loopback although RCCL is available"


# ---- plaintext operands and many-operand forms, against the real reference
@pytest.mark.parametrize("scheme,n,bits,tb,batch", [
    ("ckks", 4096, [40, 30, 30, 40], 0, 2),
    ("ckks", 16384, [60, 50, 50, 60], 0, 2),
    ("bfv", 1024, [40, 40, 41], 16, 2),
    ("bfv", 128, [30, 30, 30], 40, 2),      # t above every q_i: no fast plain lift
    ("bfv", 8192, [50, 55, 56, 60], 20, 1),
    ("bgv", 8192, [50, 55, 56, 60], 20, 1),
])
def test_plain_operands_and_many(gpu, scheme, n, bits, tb, batch):
    if not R.available():
        pytest.skip("needs the real reference (oracle/_ref)")
    primes = coeff_modulus_create(n, bits)
    t = plain_modulus_batching(n, tb) if tb else 0
    P.case_plain_ops(scheme, n, primes, t, batch=batch)


# The rounding divisions where the two-pass engine does not run (ntt_kernels.hip: ntt_epilogue): K = 2 at N = 2, 64 and 4096; the key
# switch's tail takes its plane from the low bit of the outer index: batch 1 and batch 3
@pytest.mark.parametrize("n,bits,batch,steps", [(2, [30, 30, 30], 1, ()), (64, [40, 30, 40], 3, (1,)), (4096, [50, 40, 50], 1, (1,))])
def test_rounding_epilogues_small_rings(gpu, n, bits, batch, steps):
    P.case_ckks_pipeline(n, bits, batch=batch, steps=steps, check_transforms=False)


# ... and shl_rns_stage's rounding division over an odd number of polynomials; N = 8192: the fused epilogue
@pytest.mark.parametrize("n,bits", [(2, [30, 30, 30]), (64, [40, 30, 40]), (4096, [50, 40, 50]), (1024, [50, 40, 40, 50]), (8192, [50, 40, 40, 50])])
def test_rns_stage_divide_ntt(gpu, n, bits):
    P.case_rns_stage_divide_ntt(n, bits, polys=3)


def test_rns_stages(gpu):
    primes, t = P.default_bfv_params(2048, [50, 50, 50, 50], 20)
    P.case_rns_stages(2048, primes, t)


# ---- golden vectors produced by the real reference (tests/golden/make_golden.py)
def test_golden_ckks(gpu):
    S = gpu
    g = np.load(os.path.join(GOLDEN, "ckks_n64.npz"))
    n, primes = int(g["n"]), [int(x) for x in g["primes"]]
    d = DeviceSide("ckks", n, primes)
    assert [d.ctx.ntt_root(i) for i in range(len(primes))] == [int(x) for x in g["roots"]]
    d.rlk = S.RelinKeys(d.ctx)
    d.rlk.set_key(0, g["relin_key"])
    d.glk = S.GaloisKeys(d.ctx)
    elt = int(g["galois_elt"])
    d.glk.set_key(S.GaloisKeys.get_index(elt), g["galois_key"])
    K = len(primes) - 1
    x, y = d.ct(g["a"], scale=2.0 ** 10), d.ct(g["b"], scale=2.0 ** 10)
    d.ev.multiply_inplace(x, y)
    assert np.array_equal(d.out(x)[0], g["multiply"])
    d.ev.relinearize_inplace(x, d.rlk)
    assert np.array_equal(d.out(x)[0], g["relinearize"])
    x.set_scale(float(primes[K - 1]) * 2.0 ** 10)
    d.ev.rescale_to_next_inplace(x)
    assert np.array_equal(d.out(x)[0], g["rescale"])
    assert x.scale() == float(g["rescale_scale"])
    d.ev.rotate_vector_inplace(x, 1, d.glk)
    assert np.array_equal(d.out(x)[0], g["rotate1"])
    d.ev.mod_switch_to_next_inplace(x)
    assert np.array_equal(d.out(x)[0], g["mod_switch"])


@pytest.mark.parametrize("name", ["ckks_n8192_fp_and_int", "ckks_n16384_50bit"])
def test_golden_engine_digests(gpu, name):
    """two-pass engine + fused key switch against SHA-256 digests of the real reference's outputs"""
    P.case_golden_engine(name)


def test_golden_bfv(gpu):
    S = gpu
    g = np.load(os.path.join(GOLDEN, "bfv_n32.npz"))
    n, primes, t = int(g["n"]), [int(x) for x in g["primes"]], int(g["t"])
    d = DeviceSide("bfv", n, primes, t)
    K = len(primes) - 1
    assert d.ctx.base_bsk(d.chain_index_for_K(K)) == [int(x) for x in g["bsk"]]
    d.rlk = S.RelinKeys(d.ctx)
    d.rlk.set_key(0, g["relin_key"])
    d.glk = S.GaloisKeys(d.ctx)
    elt = int(g["galois_elt"])
    d.glk.set_key(S.GaloisKeys.get_index(elt), g["galois_key"])
    d.glk.set_key(S.GaloisKeys.get_index(2 * n - 1), g["conj_key"])
    x, y = d.ct(g["a"]), d.ct(g["b"])
    d.ev.multiply_inplace(x, y)
    assert np.array_equal(d.out(x)[0], g["multiply"])
    d.ev.relinearize_inplace(x, d.rlk)
    assert np.array_equal(d.out(x)[0], g["relinearize"])
    d.ev.rotate_rows_inplace(x, 1, d.glk)
    assert np.array_equal(d.out(x)[0], g["rotate_rows1"])
    d.ev.rotate_columns_inplace(x, d.glk)
    assert np.array_equal(d.out(x)[0], g["rotate_columns"])
    d.ev.mod_switch_to_next_inplace(x)
    assert np.array_equal(d.out(x)[0], g["mod_switch"])


# ---- size-independent properties at full size (no oracle needed)
def test_full_size_properties(gpu):
    S = gpu
    n, bits = 65536, [60] + [50] * 14 + [60]
    primes = coeff_modulus_create(n, bits)
    L = len(primes)
    d = DeviceSide("ckks", n, primes)
    rng = np.random.default_rng(9)
    q = np.array(primes, dtype=np.uint64)[None, :, None]
    a = np.stack([rng.integers(0, primes[i], n, dtype=np.uint64) for i in range(L)])[None]
    b = np.stack([rng.integers(0, primes[i], n, dtype=np.uint64) for i in range(L)])[None]
    both = np.concatenate([a, b, (a + b) % q])
    buf = S.DeviceBuffer.from_numpy(both)
    S.ntt_forward(d.ctx, buf, 3, L)
    f = buf.to_numpy(both.shape)
    assert np.array_equal((f[0] + f[1]) % q[0], f[2]), "NTT is linear"
    S.ntt_inverse(d.ctx, buf, 3, L)
    assert np.array_equal(buf.to_numpy(both.shape), both), "INTT(NTT(x)) == x at N=65536, 16 primes"
    # negacyclic convolution theorem on one prime: NTT^-1(NTT(a) . NTT(x)) = a * x mod (X^N + 1), x = X
    x1 = np.zeros((1, L, n), dtype=np.uint64)
    x1[0, :, 1] = 1
    ba, bx, br = S.DeviceBuffer.from_numpy(a), S.DeviceBuffer.from_numpy(x1), S.DeviceBuffer(a.size)
    S.ntt_forward(d.ctx, ba, 1, L)
    S.ntt_forward(d.ctx, bx, 1, L)
    S.dyadic_product(d.ctx, ba, bx, br, 1, L)
    S.ntt_inverse(d.ctx, br, 1, L)
    prod = br.to_numpy(a.shape)
    shifted = np.roll(a, 1, axis=2)
    shifted[0, :, 0] = (q[0, :, 0] - a[0, :, n - 1]) % q[0, :, 0]
    assert np.array_equal(prod, shifted), "multiplication by X is a negacyclic shift"


def test_batch_items_are_independent(gpu):
    """A batch must equal the same operations applied to each ciphertext alone (ragged sizes too)."""
    n, bits = 4096, [50, 40, 40, 50]
    primes = coeff_modulus_create(n, bits)
    K = len(primes) - 1
    o = Oracle("ckks", n, primes, kind="port")
    d = DeviceSide("ckks", n, primes)
    d.upload_keys(o)
    rng = np.random.default_rng(10)
    xs = [rand_ct(rng, primes, K, n) for _ in range(7)]
    ys = [rand_ct(rng, primes, K, n) for _ in range(7)]

    def run(xl, yl):
        cx, cy = d.ct(xl, scale=2.0 ** 10), d.ct(yl, scale=2.0 ** 10)
        d.ev.multiply_inplace(cx, cy)
        d.ev.relinearize_inplace(cx, d.rlk)
        cx.set_scale(float(primes[K - 1]) * 2.0 ** 10)
        d.ev.rescale_to_next_inplace(cx)
        return d.out(cx)

    whole = run(xs, ys)
    for i in (0, 3, 6):
        assert np.array_equal(run([xs[i]], [ys[i]])[0], whole[i])


# ---- one semantic end-to-end check per scheme (needs the real reference for encrypt/decrypt)
@pytest.mark.skipif(not R.available(), reason="needs oracle/_ref for encode/encrypt/decrypt")
def test_semantic_ckks_multiply_relin_rescale(gpu):
    """CKKSEncryptMultiplyRelinRescaleDecrypt (native/tests/seal/evaluator.cpp:3513): encrypt with the
    reference, evaluate on the GPU, decrypt with the reference, |error| < 0.5 (the reference's bound)."""
    S = gpu
    n, bits = 8192, [60, 40, 40, 60]
    primes = R.coeff_modulus_create(n, bits)
    ref = R.RefContext("ckks", n, primes)
    ref.keygen_relin()
    d = DeviceSide("ckks", n, primes)
    d.rlk = S.RelinKeys(d.ctx)
    d.rlk.set_key(0, ref.key("relin", 0))
    rng = np.random.default_rng(11)
    v1, v2 = rng.uniform(-8, 8, n // 2), rng.uniform(-8, 8, n // 2)
    scale = 2.0 ** 40
    e1, e2 = ref.ckks_encrypt(v1, scale), ref.ckks_encrypt(v2, scale)
    x, y = d.ct(e1.data(), scale=scale), d.ct(e2.data(), scale=scale)
    d.ev.multiply_inplace(x, y)
    d.ev.relinearize_inplace(x, d.rlk)
    d.ev.rescale_to_next_inplace(x)
    back = ref.ct(x.chain_index(), d.out(x)[0], True, x.scale())
    got = ref.ckks_decrypt(back, n // 2)
    assert np.max(np.abs(got - v1 * v2)) < 0.5


@pytest.mark.skipif(not R.available(), reason="needs oracle/_ref for encode/encrypt/decrypt")
def test_semantic_bfv_multiply_rotate(gpu):
    """BFVEncryptMultiplyDecrypt / BFVEncryptRotateMatrixDecrypt (evaluator.cpp:1356, 5670)."""
    S = gpu
    n = 4096
    primes = R.bfv_default(n)
    t = R.plain_modulus_batching(n, 20)
    ref = R.RefContext("bfv", n, primes, t)
    ref.keygen_relin()
    elt = ref.galois_elt_from_step(1)
    ref.keygen_galois_elts([elt])
    d = DeviceSide("bfv", n, primes, t)
    d.rlk = S.RelinKeys(d.ctx)
    d.rlk.set_key(0, ref.key("relin", 0))
    d.glk = S.GaloisKeys(d.ctx)
    d.glk.set_key(S.GaloisKeys.get_index(elt), ref.key("galois", (elt - 1) >> 1))
    rng = np.random.default_rng(12)
    v1, v2 = rng.integers(0, 1000, n, dtype=np.uint64), rng.integers(0, 1000, n, dtype=np.uint64)
    e1, e2 = ref.batch_encrypt(v1), ref.batch_encrypt(v2)
    x, y = d.ct(e1.data()), d.ct(e2.data())
    d.ev.multiply_inplace(x, y)
    d.ev.relinearize_inplace(x, d.rlk)
    d.ev.rotate_rows_inplace(x, 1, d.glk)
    back = ref.ct(x.chain_index(), d.out(x)[0], False)
    got = ref.batch_decrypt(back, n)
    prod = (v1 * v2) % np.uint64(t)
    half = n // 2
    expect = np.concatenate([np.roll(prod[:half], -1), np.roll(prod[half:], -1)])
    assert np.array_equal(got, expect)


def test_oracle_kind_is_reported(gpu):
    print("oracle kind used for GPU parity:", kind_available())


def test_concurrent_calls_on_different_ciphertexts(gpu):
    """seal::Evaluator may be called concurrently on different ciphertexts (evaluator.h:79-87; ciphertext.h:48-51 only
    forbids sharing one object): four host threads run multiply + relinearize + rescale + rotate on their own
    ciphertexts through ONE evaluator and must get the results of the sequential run."""
    import threading
    S = gpu
    n, bits = 8192, [60, 40, 40, 50, 60]
    primes = coeff_modulus_create(n, bits)
    K = len(primes) - 1
    o = Oracle("ckks", n, primes, galois_elts=[3])
    d = DeviceSide("ckks", n, primes)
    d.upload_keys(o)
    rng = np.random.default_rng(77)
    inputs = [(rand_ct(rng, primes, K, n), rand_ct(rng, primes, K, n)) for _ in range(4)]

    def pipeline(a, b):
        x, y = d.ct(a, scale=2.0 ** 10), d.ct(b, scale=2.0 ** 10)
        d.ev.multiply_inplace(x, y)
        d.ev.relinearize_inplace(x, d.rlk)
        x.set_scale(float(primes[K - 1]) * 2.0 ** 10)
        d.ev.rescale_to_next_inplace(x)
        d.ev.rotate_vector_inplace(x, 1, d.glk)
        return d.out(x)[0]

    want = [pipeline(a, b) for a, b in inputs]
    got = [[None] * 6 for _ in inputs]
    errors = []

    def worker(i):
        try:
            for r in range(6):
                got[i][r] = pipeline(*inputs[i])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(inputs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(len(inputs)):
        for r in range(6):
            assert np.array_equal(got[i][r], want[i]), "thread %d repetition %d differs from the sequential result" % (i, r)


# hipGraph capture: a recorded multiply + relinearize + rescale (+ rotate) replays bit-exactly on refreshed operands
@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 2), (65536, [60] + [50] * 14 + [60], 1)])
def test_graph_capture_replay(gpu, n, bits, batch):
    import numpy as np
    import seal_amd as S
    from harness import DeviceSide
    from oracle import Oracle, coeff_modulus_create, rand_ct
    primes = coeff_modulus_create(n, bits)
    K = len(primes) - 1
    probe = Oracle("ckks", n, primes)
    elt = probe.galois_elt_from_step(1)
    o = Oracle("ckks", n, primes, galois_elts=[elt])
    d = DeviceSide("ckks", n, primes)
    d.upload_keys(o)
    rng = np.random.default_rng(21)
    scale = 2.0 ** 20

    def expected(x, y):
        r = o.rescale(o.relinearize(o.multiply(x, y)))
        return o.apply_galois(r, elt)

    xs = [rand_ct(rng, primes, K, n) for _ in range(batch)]
    ys = [rand_ct(rng, primes, K, n) for _ in range(batch)]
    cx, cy = d.ct(xs, scale=scale), d.ct(ys, scale=scale)
    work = S.Ciphertext(d.ctx, batch=batch)

    def step():
        d.ev.multiply(cx, cy, work)
        d.ev.relinearize_inplace(work, d.rlk)
        work.set_scale(float(primes[K - 1]) * scale)
        d.ev.rescale_to_next_inplace(work)
        d.ev.rotate_vector_inplace(work, 1, d.glk)

    step()  # eager once
    eager = d.out(work)
    for b in range(batch):
        assert np.array_equal(eager[b], expected(xs[b], ys[b]))
    graph = d.ev.capture(step)
    for trial in range(3):
        if trial:
            xs = [rand_ct(rng, primes, K, n) for _ in range(batch)]
            ys = [rand_ct(rng, primes, K, n) for _ in range(batch)]
            cx.load(np.stack(xs, axis=1))
            cy.load(np.stack(ys, axis=1))
        graph.launch()
        got = d.out(work)
        assert work.size() == 2 and work.coeff_modulus_size() == K - 1
        for b in range(batch):
            assert np.array_equal(got[b], expected(xs[b], ys[b])), "graph replay %d item %d" % (trial, b)
    # capturing with the read-back check on is refused, and nesting too
    d.ev.set_transparent_check(True)
    with pytest.raises(S.LogicError):
        d.ev.capture(step)
    d.ev.set_transparent_check(False)


@pytest.mark.parametrize("scheme,n,bits", [("ckks", 4096, [54, 42, 55]), ("ckks", 16384, [60, 50, 50, 60]), ("bgv", 8192, [50, 40, 56]),
                                            ("bfv", 4096, [36, 36, 37])])
def test_product_growth(gpu, scheme, n, bits):
    """the 2 x 2 product into a new slab and in place, distinct operands and squares, three items"""
    for seed in (51, 52, 53):
        P.case_product_growth(scheme, n, bits, seed=seed)


@pytest.mark.parametrize("groups", ["auto", "1"])
def test_deferred_tail_two_readers(gpu, monkeypatch, groups):
    """two threads read one ciphertext whose key-switch tail is pending: it runs once, both see the completed words;
    groups "1": the digits as one group (ks2 itself leaves c + S P^-1 behind: KsFusedArgs::fold_c0)"""
    if groups != "auto":
        monkeypatch.setenv("SEALHIP_KS_SPLIT", groups)
    P.case_deferred_tail_two_readers(8192, (50, 40, 40, 60), rounds=8)
    P.case_deferred_tail_two_readers(65536, (60, 50, 50, 60), rounds=3)


def test_device_field_check(gpu):
    """the integer back end's gfx950 instruction sequences (field.h: products issued through single-instruction wrappers, device
    only) against 128-bit arithmetic on the device itself: tests/device_field_check.hip, built by seal_amd/csrc/Makefile"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seal_amd", "lib", "device_field_check")
    assert os.path.exists(exe), "seal_amd/lib/device_field_check is not built (make -C seal_amd/csrc gpu)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "device_field_check ok" in out.stdout, out.stdout + out.stderr


def test_device_fp_field_check(gpu):
    """the double-precision back end and the phase templates that place its range reductions, at the bounds field.h documents,
    compiled with the library's flags and compared with 128-bit arithmetic on the device itself (tests/device_fp_field_check.hip,
    the case body of tests/fp_field_cases.h); every double it produces on the streams it shares with the host check has the
    host's bits (tests/golden/fp_field_digest.json, written by tests/field_check.cpp)"""
    import json
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "seal_amd", "lib", "device_fp_field_check")
    assert os.path.exists(exe), "seal_amd/lib/device_fp_field_check is not built (make -C seal_amd/csrc gpu)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "device_fp_field_check ok" in out.stdout, out.stdout + out.stderr
    digest = re.search(r"^device_fp_field_check digest ([0-9a-f]{16})$", out.stdout, re.M)
    assert digest, out.stdout
    with open(os.path.join(root, "tests", "golden", "fp_field_digest.json")) as f:
        assert digest.group(1) == json.load(f)["digest"], out.stdout


def test_mod_reduce(gpu):
    import sealref
    if not sealref.available():
        pytest.skip("oracle/_ref did not travel")
    P.case_mod_reduce(16384, [60, 50, 50, 50, 60])


@pytest.mark.parametrize("n,bits", [(8192, [60, 30, 30, 30, 40, 60]), (16384, [60, 50, 50, 50, 50, 60]), (65536, [60, 50, 40, 50, 60, 50, 60]), (4096, [36, 30, 30, 30, 36])])
def test_multi_level_forms_ckks(gpu, n, bits):
    """rescale_to_inplace / mod_switch_to_inplace(Ciphertext) over three levels against the reference's own multi-level calls
    (evaluator.cpp:1451-1473, 1543-1595), directly and with a key switch's deferred tail pending (tail counters asserted)"""
    import sealref
    if not sealref.available():
        pytest.skip("oracle/_ref did not travel")
    P.case_multi_level_ckks(n, bits, batch=3 if n <= 16384 else 1)


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_multi_level_forms_bfv_bgv(gpu, scheme):
    import sealref
    from oracle import coeff_modulus_create, plain_modulus_batching
    if not sealref.available():
        pytest.skip("oracle/_ref did not travel")
    n = 16384
    P.case_multi_level_bfv_bgv(scheme, n, coeff_modulus_create(n, [55, 55, 50, 58, 60, 55]), plain_modulus_batching(n, 20), batch=3)


# ---- streams: non-blocking streams, out-of-place forms in a captured graph, two evaluators sharing the pool
def _ckks_setup(n, bits, galois=True):
    import numpy as np
    from harness import DeviceSide
    from oracle import Oracle, coeff_modulus_create
    primes = coeff_modulus_create(n, bits)
    probe = Oracle("ckks", n, primes)
    elt = probe.galois_elt_from_step(1)
    o = Oracle("ckks", n, primes, galois_elts=[elt] if galois else [])
    d = DeviceSide("ckks", n, primes)
    d.upload_keys(o)
    return primes, o, d, elt


def test_non_blocking_stream_parity(gpu):
    """the whole pipeline on a hipStreamNonBlocking stream (what a PyTorch stream is), out-of-place forms included: the
    destination copy runs on the evaluator's stream, not on the NULL stream"""
    import numpy as np
    import seal_amd as S
    from oracle import rand_ct
    n, bits = 8192, [60, 40, 40, 60]
    primes, o, d, elt = _ckks_setup(n, bits)
    K = len(primes) - 1
    stream = S.Stream(non_blocking=True)
    d.ev.set_stream(stream.handle)
    rng = np.random.default_rng(5)
    for trial in range(6):
        x, y = rand_ct(rng, primes, K, n), rand_ct(rng, primes, K, n)
        cx, cy = d.ct([x], scale=2.0 ** 10), d.ct([y], scale=2.0 ** 10)
        prod, rel, res = S.Ciphertext(d.ctx), S.Ciphertext(d.ctx), S.Ciphertext(d.ctx)
        d.ev.multiply(cx, cy, prod)
        d.ev.relinearize(prod, d.rlk, rel)              # destination != source: copy + operation on `stream`
        rel.set_scale(float(primes[K - 1]) * 2.0 ** 10)
        d.ev.rescale_to_next(rel, res)
        d.ev.rotate_vector_inplace(res, 1, d.glk)
        exp = o.apply_galois(o.rescale(o.relinearize(o.multiply(x, y))), elt)
        assert np.array_equal(d.out(res)[0], exp), "trial %d" % trial
    d.ev.set_stream(None)


def test_graph_capture_out_of_place_forms(gpu):
    """a recorded sequence of destination forms (square -> relinearize -> rescale, each into its own object) replays on
    refreshed operands: the destination copies are part of the graph"""
    import numpy as np
    import seal_amd as S
    from oracle import rand_ct
    n, bits = 8192, [60, 40, 40, 60]
    primes, o, d, elt = _ckks_setup(n, bits, galois=False)
    K = len(primes) - 1
    rng = np.random.default_rng(6)
    x = rand_ct(rng, primes, K, n)
    cx = d.ct([x], scale=2.0 ** 10)
    sq, rel, res = S.Ciphertext(d.ctx), S.Ciphertext(d.ctx), S.Ciphertext(d.ctx)

    def step():
        d.ev.square(cx, sq)
        d.ev.relinearize(sq, d.rlk, rel)
        rel.set_scale(float(primes[K - 1]) * 2.0 ** 10)
        d.ev.rescale_to_next(rel, res)

    def expected(v):
        return o.rescale(o.relinearize(o.multiply(v, v)))

    step()
    assert np.array_equal(d.out(res)[0], expected(x))
    graph = d.ev.capture(step)
    for trial in range(3):
        x = rand_ct(rng, primes, K, n)
        cx.load(x[:, None])
        graph.launch()
        assert np.array_equal(d.out(res)[0], expected(x)), "replay %d" % trial
    # the graph owns the scratch it recorded: eager work in between must not disturb a later replay
    other = d.ct([rand_ct(rng, primes, K, n)], scale=2.0 ** 10)
    d.ev.square_inplace(other)
    d.ev.relinearize_inplace(other, d.rlk)
    graph.launch()
    assert np.array_equal(d.out(res)[0], expected(x))
    del graph


def test_two_evaluators_two_streams_share_the_pool(gpu):
    """two evaluators on two non-blocking streams issue interleaved work from one host thread; the scratch blocks one frees are
    handed to the other (same sizes), so the pool has to order the streams; every result equals the reference's"""
    import numpy as np
    import seal_amd as S
    from oracle import rand_ct
    n, bits = 16384, [60, 50, 50, 50, 60]
    primes, o, d, elt = _ckks_setup(n, bits, galois=False)
    K = len(primes) - 1
    ev2 = S.Evaluator(d.ctx)
    s1, s2 = S.Stream(True), S.Stream(True)
    d.ev.set_stream(s1.handle)
    ev2.set_stream(s2.handle)
    rng = np.random.default_rng(8)
    batch = 8
    waits0 = S.pool_stats()[1]
    xs = [[rand_ct(rng, primes, K, n) for _ in range(batch)] for _ in range(2)]
    ys = [[rand_ct(rng, primes, K, n) for _ in range(batch)] for _ in range(2)]
    cts = [(d.ct(xs[i], scale=2.0 ** 10), d.ct(ys[i], scale=2.0 ** 10)) for i in range(2)]
    outs = [S.Ciphertext(d.ctx, batch=batch) for _ in range(2)]
    evs = [d.ev, ev2]
    for rnd in range(4):
        for i in range(2):          # no host synchronisation between the two evaluators' calls
            evs[i].multiply(cts[i][0], cts[i][1], outs[i])
            evs[i].relinearize_inplace(outs[i], d.rlk)
        for i in range(2):
            got = d.out(outs[i])
            for b in range(batch):
                assert np.array_equal(got[b], o.relinearize(o.multiply(xs[i][b], ys[i][b]))), "round %d evaluator %d item %d" % (rnd, i, b)
    assert S.pool_stats()[1] > waits0, "scratch never changed stream: the test did not exercise the ordering"
    d.ev.set_stream(None)
    ev2.set_stream(None)


@pytest.mark.parametrize("groups", ["auto", "1"])
def test_deferred_tail_lifecycle(gpu, monkeypatch, groups):
    """deferred key-switch tails (sealhip.h): folded into a rescale by their owner, completed by anyone else who needs the words;
    at N = 8192 and at the headline size; groups "1": the digits as one group (ks2 itself adds the ciphertext's words: KsFusedArgs::fold_c0)"""
    if groups != "auto":
        monkeypatch.setenv("SEALHIP_KS_SPLIT", groups)
    P.case_deferred_tail_lifecycle()
    P.case_deferred_tail_lifecycle(65536, (60, 50, 50, 50, 60))
