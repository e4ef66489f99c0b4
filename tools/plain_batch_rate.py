"""One plaintext per item of a device-resident batch against one plaintext for all of it, at the headline parameters
(CKKS, N = 65536, {60, 14x50, 60}, batch 256, size 2), in place:

  device     Evaluator.multiply_plain_device / add_plain_device - [batch][K][N] plaintext words (CKKSEncoder.encode_device)
  broadcast  Evaluator.multiply_plain_inplace / add_plain_inplace of the same build on the same ciphertext with one Plaintext
             handle: the yardstick.  By bytes the per-item multiply moves 2 size + 1 planes where the broadcast form moves 2 size,
             and the per-item add moves 3 planes of one polynomial where the broadcast form moves 2.

The four calls are interleaved repetition by repetition, HIP events on the evaluator's (NULL) stream around each call, one warm-up
round first; median and range per cell, achieved GB/s from the bytes above, the measured ratio device / broadcast next to the byte
ratio, and the spread the broadcast form shows against itself (max / min over the repetitions).

BFV at N = 32768, 14 x 55 bits, batch 128 (reported only): multiply_plain_device coefficient form x coefficient form against the same
call with plaintexts that Evaluator.transform_plain_to_ntt_device lifted and transformed beforehand.

  python tools/plain_batch_rate.py [--batch 256] [--bfv-batch 128] [--reps 10] [--only-device] [--out FILE] [--small] [--lib PATH]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import seal_amd as S
from harness import DeviceSide
from oracle import coeff_modulus_create, plain_modulus_batching

N, BITS = 65536, [60] + [50] * 14 + [60]
BFV_N, BFV_BITS = 32768, [55] * 14


def interleaved(fns, reps):
    """{name: [ms]}: every repetition times each call once, in turn"""
    for _, prepare, fn in fns:
        prepare()
        fn()
    S.device_synchronize()
    tm, out = S.HipTimer(), {name: [] for name, _, _ in fns}
    for _ in range(reps):
        for name, prepare, fn in fns:
            prepare()
            tm.start()
            fn()
            out[name].append(tm.stop())
    return out


def cell(ms, nbytes):
    med = float(np.median(ms))
    return "%8.3f [%8.3f .. %8.3f] ms  %7.1f GB/s" % (med, min(ms), max(ms), nbytes / max(med, 1e-9) / 1e6)


def ckks(a, lines):
    d = DeviceSide("ckks", N, coeff_modulus_create(N, BITS))
    kg = S.KeyGenerator(d.ctx)
    enc = S.Encryptor(d.ctx, kg.secret_key())
    coder = S.CKKSEncoder(d.ctx)
    pid, scale, batch = d.ctx.first_parms_id(), 2.0 ** 40, a.batch
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    rng = np.random.default_rng(1)
    words = coder.encode_device(S.DeviceBuffer.from_array(rng.standard_normal((batch, N // 2))), batch, pid, scale)
    ct = enc.encrypt_symmetric_device(words, batch, pid, scale)
    one = S.Plaintext(d.ctx).set_from_device(words, K * N, offset=0, parms_id=pid, scale=scale)
    plane = batch * K * N * 8   # bytes of one polynomial of the batch
    reset = lambda: ct.set_scale(scale)
    fns = [("multiply device", reset, lambda: d.ev.multiply_plain_device(ct, words, True, scale)),
           ("add device", reset, lambda: d.ev.add_plain_device(ct, words, True, scale))]
    if not a.only_device:
        fns += [("multiply broadcast", reset, lambda: d.ev.multiply_plain_inplace(ct, one)),
                ("add broadcast", reset, lambda: d.ev.add_plain_inplace(ct, one))]
    ms = interleaved(fns, a.reps)
    nbytes = {"multiply device": 5 * plane, "multiply broadcast": 4 * plane, "add device": 3 * plane, "add broadcast": 2 * plane}
    lines.append("CKKS N = %d, K = %d, batch %d, size 2, in place; median [min .. max] of %d interleaved repetitions (HIP events)" % (N, K, batch, a.reps))
    for name, _, _ in fns:
        lines.append("  %-20s %s" % (name, cell(ms[name], nbytes[name])))
    if not a.only_device:
        for op in ("multiply", "add"):
            dev, bc = ms[op + " device"], ms[op + " broadcast"]
            lines.append("  %-8s device / broadcast: measured %.3f, by bytes %.3f; the broadcast form against itself: max / min = %.3f"
                         % (op, np.median(dev) / max(np.median(bc), 1e-9), nbytes[op + " device"] / nbytes[op + " broadcast"], max(bc) / max(min(bc), 1e-9)))


def bfv(a, lines):
    t = plain_modulus_batching(BFV_N, 20)
    d = DeviceSide("bfv", BFV_N, coeff_modulus_create(BFV_N, BFV_BITS), t)
    kg = S.KeyGenerator(d.ctx)
    enc = S.Encryptor(d.ctx, kg.secret_key())
    pid, batch = d.ctx.first_parms_id(), a.bfv_batch
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    rng = np.random.default_rng(2)
    coeffs = S.DeviceBuffer.from_numpy(rng.integers(0, t, (batch, BFV_N), dtype=np.uint64))
    ct = enc.encrypt_symmetric_device(coeffs, batch, pid)
    pre = d.ev.transform_plain_to_ntt_device(coeffs, batch, pid)
    nothing = lambda: None
    ms = interleaved([("coefficient plaintexts", nothing, lambda: d.ev.multiply_plain_device(ct, coeffs, False)),
                      ("pre-transformed", nothing, lambda: d.ev.multiply_plain_device(ct, pre, True))], a.reps)
    lines.append("BFV N = %d, K = %d, batch %d, size 2, coefficient-form ciphertext, in place; ms per call: median [min .. max]" % (BFV_N, K, batch))
    for name in ("coefficient plaintexts", "pre-transformed"):
        lines.append("  %-24s %8.3f [%8.3f .. %8.3f]" % (name, float(np.median(ms[name])), min(ms[name]), max(ms[name])))
    lines.append("  transform_plain_to_ntt_device beforehand saves %.3f ms per call (%.1f %%)"
                 % (np.median(ms["coefficient plaintexts"]) - np.median(ms["pre-transformed"]),
                    100.0 * (1 - np.median(ms["pre-transformed"]) / max(np.median(ms["coefficient plaintexts"]), 1e-9))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bfv-batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-device", action="store_true", help="the per-item CKKS forms alone (for a kernel trace)")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, short chains: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    a = ap.parse_args()
    global N, BITS, BFV_N, BFV_BITS
    if a.small:
        N, BITS, BFV_N, BFV_BITS = 1024, [60, 40, 60], 1024, [36, 36, 37]
    S.load(a.lib)
    lines = []
    ckks(a, lines)
    if not a.only_device:
        bfv(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
