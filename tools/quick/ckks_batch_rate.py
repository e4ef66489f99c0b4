"""CKKSEncoder on whole batches in HBM (encode_device / decode_device) next to a loop of the per-object calls over the same
items, at C5 (N = 65536, {60, 14x50, 60}) and N = 16384 ({60, 4x50, 60}), batch 1, 16 and 256, first data level, scale 2^40.
Batched forms: the inputs are already in HBM and the timed region has no host copies (each call returns after its work is
done).  Per-object loop: encode(host vector) -> Plaintext and decode(Plaintext) -> host vector, copies included, as a client
calls them.  Median over repeated runs, ms per call and per item.
--profile: only one batch-256 encode and one batch-256 decode at C5 after a warm-up (for rocprofv3 --kernel-trace --stats)."""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import seal_amd as S
from harness import DeviceSide
from oracle import coeff_modulus_create

SIZES = (("C5", 65536, [60] + [50] * 14 + [60]), ("N16384", 16384, [60] + [50] * 4 + [60]))
SCALE = 2.0 ** 40


def median_ms(fn, reps):
    fn()
    S.device_synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        S.device_synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def setup(n, bits, batch):
    d = DeviceSide("ckks", n, coeff_modulus_create(n, bits), 0)
    enc = S.CKKSEncoder(d.ctx)
    pid = d.ctx.first_parms_id()
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    x = np.random.default_rng(1).standard_normal((batch, n // 2))
    return d, enc, pid, K, x


def profile():
    n, bits = SIZES[0][1], SIZES[0][2]
    d, enc, pid, K, x = setup(n, bits, 256)
    xb, words, vals = S.DeviceBuffer.from_array(x), S.DeviceBuffer(256 * K * n), S.DeviceBuffer(256 * n // 2)
    enc.encode_device(xb, 1, pid, SCALE, count=n // 2, out=words)        # warm-up: tables, pool
    enc.decode_device(words, 1, pid, SCALE, out=vals)
    S.device_synchronize()
    enc.encode_device(xb, 256, pid, SCALE, count=n // 2, out=words)
    enc.decode_device(words, 256, pid, SCALE, out=vals)
    S.device_synchronize()
    print("profiled: one batch-256 encode_device and one batch-256 decode_device at C5")


def main():
    print("ms per call (per item) | batched form vs a loop of per-object calls | speed-up per item")
    for name, n, bits in SIZES:
        d, enc, pid, K, x = setup(n, bits, 256)
        xb, words, vals = S.DeviceBuffer.from_array(x), S.DeviceBuffer(256 * K * n), S.DeviceBuffer(256 * n // 2)
        pts = [enc.encode(x[b], pid, SCALE) for b in range(256)]
        for batch in (1, 16, 256):
            reps = 9 if batch < 256 else 5
            e_dev = median_ms(lambda: enc.encode_device(xb, batch, pid, SCALE, count=n // 2, out=words), reps)
            d_dev = median_ms(lambda: enc.decode_device(words, batch, pid, SCALE, out=vals), reps)
            e_obj = median_ms(lambda: [enc.encode(x[b], pid, SCALE) for b in range(batch)], 3 if batch == 256 else reps)
            d_obj = median_ms(lambda: [enc.decode(pts[b]) for b in range(batch)], 3 if batch == 256 else reps)
            for what, dev, obj in (("encode", e_dev, e_obj), ("decode", d_dev, d_obj)):
                print("%-7s N=%-6d K=%-2d batch %3d  %s_device %9.3f (%7.4f) | per-object loop %9.3f (%7.4f) | x%.1f"
                      % (name, n, K, batch, what, dev, dev / batch, obj, obj / batch, obj / dev), flush=True)


if __name__ == "__main__":
    profile() if "--profile" in sys.argv else main()
