"""Digit-parallel key switching over real GPUs: one process per GPU, the library's own RCCL communicator,
both exchange shapes, keys distributed by the library's broadcast; every rank's result equals the reference's.  Needs at
least two MI355X in the box - skipped on the single-GPU boxes; the ranks-emulated and one-rank-RCCL forms of the same
arithmetic run everywhere (test_gpu_parity.py: test_digit_parallel_*)."""
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", [0, 1])
def test_digit_parallel_over_real_ranks(gpu, exchange):
    import seal_amd as S
    n_dev = S.device_count()
    if n_dev < 2:
        pytest.skip("one GPU visible: the multi-rank RCCL path needs at least two")
    if not S.Comm.rccl_available():
        pytest.fail("librccl.so.1 did not load on a multi-GPU box")
    nranks = min(n_dev, 8)
    with tempfile.TemporaryDirectory() as tmp:
        id_path = os.path.join(tmp, "rccl_id")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "multi_gpu_worker.py"), str(r), str(nranks), id_path, str(exchange)],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(nranks)]
        outs = []
        for p in procs:
            try:
                out, _ = p.communicate(timeout=900)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    for r, out in enumerate(outs):
        assert "MULTI_GPU_OK rank=%d/%d exchange=%d" % (r, nranks, exchange) in out, out[-1500:]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,extra", [("headline", ["--batch", "8"]), ("bfv_c4", ["--total-batch", "16"]),
                                            ("rotate_c5", ["--batch", "2", "--exchange", "reduce_scatter"])])
def test_bench_over_real_ranks(gpu, workload, extra):
    """`python bench.py --gpus 2 --full` on real GPUs: the launcher starts one rank per GPU, the probe all-reduce reaches both
    over RCCL (rccl_ranks in the line), every rank's sampled items equal the reference's, every rank reports its own rate.  Batch
    sharding for the headline and configs[3], the digit-parallel exchange inside the library for configs[4]."""
    import json
    import seal_amd as S
    if S.device_count() < 2:
        pytest.skip("one GPU visible: the multi-rank bench needs at least two")
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload", workload,
                          "--full", "--no-cpu-baseline", "--no-pmc"] + extra, env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["collective_backend"] == "nccl", line
    assert [p["rank"] for p in line["per_rank"]] == [0, 1] and all(p["value"] > 0 for p in line["per_rank"])
    assert line["value"] > 0 and line["verified_items"] and line["verified_items"] >= 4, line
    if workload == "rotate_c5":
        assert "RCCL inside libsealhip" in line["config"]["parallelism"], line["config"]["parallelism"]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,extra", [("rotate_c5", ["--batch", "2"]), ("bfv_c4", ["--total-batch", "6"]), ("headline", ["--batch", "3"])])
def test_two_processes_share_the_one_gpu(gpu, workload, extra):
    """The only N > 1 evidence a one-GPU box can give (VERDICT r4 next #7b): `python bench.py --gpus 2 --full` with both ranks on device 0
    (SEALHIP_BENCH_SHARE_GPU=1: process group gloo, RCCL refuses two ranks on one device) and the REAL kernels - batch sharding for
    the headline and configs[3] (uneven shards: 3 + 3 of 6, 3 each), and for configs[4] the digit-parallel key switch across a real
    process boundary: each rank runs switch_key_partial on its digits, the partial sums are added by torch.distributed, each
    rank runs the *Finish kernels (deferred tail, folded into the rescale).  Every rank's sampled items equal the reference's."""
    import json
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", SEALHIP_BENCH_SHARE_GPU="1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload", workload,
                          "--full", "--no-cpu-baseline", "--no-pmc", "--no-children"] + extra, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["collective_backend"] == "gloo", line
    assert "shared_gpu" in line["config"], line["config"]
    assert [p["rank"] for p in line["per_rank"]] == [0, 1] and all(p["value"] > 0 for p in line["per_rank"])
    assert line["value"] > 0 and line["verified_items"] and line["verified_items"] >= 4, line
    assert "free" in out.stderr and "GiB free of" in out.stderr, "the per-rank memory line is missing: " + out.stderr[-800:]
    if workload == "rotate_c5":
        assert "torch.distributed" in line["config"]["parallelism"], line["config"]["parallelism"]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,extra", [("headline", ["--batch", "1"]), ("bfv_c4", ["--total-batch", "9"]), ("rotate_c5", ["--batch", "2"])])
def test_eight_processes_share_the_one_gpu(gpu, workload, extra):
    """Eight-rank first contact as far as a one-GPU box allows: `python bench.py --gpus 8 --full`, the eight ranks real
    processes with the REAL kernels on device 0 (SEALHIP_BENCH_SHARE_GPU=1, gloo).  One item per rank for the headline; 9 items over 8
    ranks for configs[3] (shards 2, 1, 1, ...); configs[4] with 15 digits over 8 ranks (2, 2, ..., 1).  Every rank pinned to its own
    CPUs, every rank's items equal the reference's.  (The ring kernel is opt-in and stays off: processes that share a GPU must not
    run workgroups that wait for each other.)"""
    import json
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SEALHIP_NTT_RING")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", SEALHIP_BENCH_SHARE_GPU="1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--workload", workload,
                          "--full", "--no-cpu-baseline", "--no-pmc", "--no-children"] + extra, env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["rccl_ranks"] == 8 and line["collective_backend"] == "gloo", line
    assert "shared_gpu" in line["config"], line["config"]
    assert [p["rank"] for p in line["per_rank"]] == list(range(8)) and all(p["value"] > 0 for p in line["per_rank"])
    assert line["value"] > 0 and line["verified_items"] and line["verified_items"] >= 8, line
    assert line["config"]["cpus_per_rank"] and line["config"]["cpus_per_rank"] >= 1
    if workload == "rotate_c5":
        assert line["latency_ms_per_ciphertext"] > 0 and "torch.distributed" in line["config"]["parallelism"]
