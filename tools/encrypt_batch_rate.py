"""Filling a batch of fresh CKKS ciphertexts at the headline parameters (N = 65536, {60, 14x50, 60}) from plaintexts that are
already in HBM (CKKSEncoder.encode_device), secret-key and public-key:

  batch    Encryptor.encrypt_symmetric_device / encrypt_device - one call for the whole batch
  loop     the per-item loop of tests/ckks_batch_cases.py::case_client_loop: Plaintext.set_from_device -> per-object encryption
           -> save_bytes -> load_bytes(item=k)   (what filled a batch before the batch forms existed)
  direct   the same loop without the save / load detour: per-object encryption + one device-to-device copy of the item
           (Ciphertext_CopyFromDevice moves whole slabs, so the copy goes to a staging ciphertext of one item: the same bytes)

HIP events on the NULL stream around each repetition (the calls return when their work is done, host-side sampling included),
`--reps` repetitions after one warm-up; median and range per cell.  Also reported: the share of the batch call spent in the
host's walk over the rejection bitmap (SealHip_XofStats).  Keys come from the device's own KeyGenerator: no reference needed.

  python tools/encrypt_batch_rate.py [--batches 1,8,64,256] [--reps 10] [--only-batch] [--out FILE] [--small] [--lib PATH]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import seal_amd as S
from harness import DeviceSide
from oracle import coeff_modulus_create

N, BITS = 65536, [60] + [50] * 14 + [60]


def timed(fn, reps):
    fn()
    S.device_synchronize()
    tm, out = S.HipTimer(), []
    for _ in range(reps):
        tm.start()
        fn()
        out.append(tm.stop())
    return out


def cell(ms):
    return "%9.2f [%8.2f .. %8.2f]" % (float(np.median(ms)), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-batch", action="store_true", help="the batch forms alone (for a kernel trace)")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, {60, 40, 60}: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    a = ap.parse_args()
    global N, BITS
    if a.small:
        N, BITS = 1024, [60, 40, 60]
    S.load(a.lib)
    d = DeviceSide("ckks", N, coeff_modulus_create(N, BITS))
    kg = S.KeyGenerator(d.ctx)
    enc = S.Encryptor(d.ctx, kg.secret_key(), public_key=kg.create_public_key())
    coder = S.CKKSEncoder(d.ctx)
    pid, scale = d.ctx.first_parms_id(), 2.0 ** 40
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    rng = np.random.default_rng(1)
    lines = ["CKKS N = %d, K = %d at the first level; ms per filled batch: median [min .. max] of %d repetitions (HIP events)" % (N, K, a.reps),
             "%-4s %5s  %-32s %-32s %-32s %s" % ("key", "batch", "batch form", "loop (save/load per item)", "direct (encrypt + D2D copy)", "host walk share")]
    for batch in [int(x) for x in a.batches.split(",")]:
        words = coder.encode_device(S.DeviceBuffer.from_array(rng.standard_normal((batch, N // 2))), batch, pid, scale)
        dest = S.Ciphertext(d.ctx, batch=batch)
        one, stage = S.Ciphertext(d.ctx), S.Ciphertext(d.ctx)
        for name, batch_fn, item_fn in (("sk", enc.encrypt_symmetric_device, enc.encrypt_symmetric), ("pk", enc.encrypt_device, enc.encrypt)):
            def plain(k):
                return S.Plaintext(d.ctx).set_from_device(words, K * N, offset=k * K * N, parms_id=pid, scale=scale)

            def loop():
                for k in range(batch):
                    dest.load_bytes(item_fn(plain(k)).save_bytes(), item=k)

            def direct():
                for k in range(batch):
                    item_fn(plain(k), destination=one)
                    if not stage.shape()[0]:
                        stage.load_bytes(one.save_bytes())
                    ptr, count = one.device_ptr()
                    stage.load_device(ptr, count)

            before = S.xof_stats()
            t_batch = timed(lambda: batch_fn(words, batch, pid, scale, destination=dest), a.reps)
            after = S.xof_stats()
            walk = (after[2] - before[2]) / 1e6 / (a.reps + 1)
            share = "%5.1f %% (%.2f ms; %d words replaced)" % (100.0 * walk / max(float(np.median(t_batch)), 1e-9), walk, after[1] - before[1])
            if a.only_batch:
                lines.append("%-4s %5d  %-32s %-32s %-32s %s" % (name, batch, cell(t_batch), "-", "-", share))
            else:
                lines.append("%-4s %5d  %-32s %-32s %-32s %s" % (name, batch, cell(t_batch), cell(timed(loop, a.reps)), cell(timed(direct, a.reps)), share))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
