"""bench.py's multi-rank branch (one process per GPU, channels sharded over ranks, barrier +
max-over-ranks timing) run for real: two ranks started by torch.distributed.run as a child process.
With two GPUs the backend is nccl (= RCCL); on a one-GPU box both ranks share the GPU over gloo."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(nproc, *extra, env_extra=None):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(env_extra or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                 # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_two_rank_bench_shards_channels():
    import torch
    backend = {} if torch.cuda.device_count() >= 2 else {"SDFT_BENCH_BACKEND": "gloo"}
    res = run_bench(2, "--steps", "2", "--warmup", "1", "--samples", "4096", "--no-extras", env_extra=backend)
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["warmup"] == 1
    assert res["config"]["channels_total"] == 128 and res["config"]["samples_per_channel"] == 4096
    assert res["scaling"] == "weak" and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["roofline"]["bound"] == "hbm" and 0 < res["roofline"]["frac"] < 1
    # value = all ranks' samples / max-over-ranks time
    assert abs(res["value"] - 128 * 4096 / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * res["value"]
    # the census that makes a multi-GPU record checkable without logs
    rk = res["ranks"]
    assert rk["ranks_in_collectives"] == 2 and rk["world_size"] == 2
    assert rk["distinct_local_devices"] == (2 if not backend else 1)
    assert rk["collective_backend"].startswith("rccl") == (not backend)
    assert 0 < rk["ms_per_step_min_over_ranks"] <= rk["ms_per_step_max_over_ranks"] <= res["ms_per_step"] * 1.001
    assert 0 < rk["roofline_frac_min_over_ranks"] <= rk["roofline_frac_max_over_ranks"] < 1


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` WITHOUT a launcher (how a driver may well call it) must come back as a 2-rank measurement or
    fail -- never as a one-rank line that says n_gpus = 1 (round-4 review).  bench.py starts torch.distributed.run as a child."""
    import torch
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    two_gpus = torch.cuda.device_count() >= 2
    if not two_gpus:
        # under RCCL it refuses (rc 2, no JSON line) ...
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--no-extras"],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 2 and not [l for l in r.stdout.splitlines() if l.startswith("{")], (r.returncode, r.stdout[-500:])
        env["SDFT_BENCH_BACKEND"] = "gloo"                      # ... the functional run shares the one GPU over gloo
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--samples", "4096", "--no-extras"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["ranks"]["ranks_in_collectives"] == 2 and res["config"]["channels_total"] == 128
    assert res["ranks"]["distinct_local_devices"] == (2 if two_gpus else 1) and "invalid" not in res
    # a launcher that started another number of ranks than --gpus says: refused
    env2 = dict(env); env2["WORLD_SIZE"] = "1"; env2["RANK"] = "0"; env2["LOCAL_RANK"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--no-extras"],
                       capture_output=True, text=True, cwd=ROOT, env=env2, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_single_rank_bench_line_contract():
    res = run_bench(1, "--steps", "2", "--warmup", "1", "--samples", "65536", "--cpu-samples", "8192", "--no-cpu-all-cores", "--full")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in res, key
    assert res["n_gpus"] == 1 and res["vs_baseline"] is None and res["dtype"] == "f64" and res["data"] == "synthetic"
    assert res["cpu_baseline"]["cores"] == 1 and res["cpu_baseline"]["value"] > 0
    assert res["analysis_plus_synthesis_msamples_s"] > 0 and res["analysis_plus_synthesis_msamples_s"] < res["value"]
    # round 4: every single-GPU BASELINE config and the single-sample entry points ride in the same line
    cfg = res["configs"]
    for key in ("config2", "config3"):
        assert "skipped" in cfg[key] or (0 < cfg[key]["forward_frac_of_peak"] < 1 and 0 < cfg[key]["inverse_frac_of_peak"] < 1), cfg[key]
    assert cfg["single_sample"]["sdft_us_per_call_device_row"] > 0 and cfg["single_sample"]["cpu_sdft_us_per_sample"] > 0
    assert res["roofline"]["traffic"] is None or "replayed" in res["roofline"]["traffic_source"]
    assert res["ranks"] is None                                                    # the census belongs to N > 1 lines
    # round 6: the output matrix comes from the library's own placement call inside matrix + 64 GiB, untimed, and the line says how it was
    # found; the same K steps into the process' first allocation ride beside the headline
    bp = res["buffer_placement"]
    assert "untimed" in bp["policy"] and "sdft_hip_malloc_matrix_in_arena" in bp["policy"] and bp["placed"] is True, bp
    assert bp["arena_bytes"] <= bp["matrix_bytes"] + (64 << 30) and bp["window_offset"] + bp["matrix_bytes"] <= bp["arena_bytes"], bp
    assert bp["window_probes"] <= 9 * bp["arenas_tried"] and bp["pair_probes"] <= 16 * bp["arenas_tried"] and bp["window_gbs"] >= bp["start_gbs"] > 0, bp
    fa = res["first_allocation"]
    assert fa["value"] > 0 and 0 < fa["frac"] < 1 and fa["ms_per_step"] > 0 and "FIRST allocation" in fa["is"], fa
    # the headline workload as asynchronous calls into two matrices in turn, pipelined against one stream on equally placed matrices
    two = res["two_matrices_in_turn"]
    assert "error" in two or (two["pipelined"]["pipelined_calls"] >= 10 and two["one_stream"]["pipelined_calls"] == 0 and
                              0 < two["pipelined"]["frac_of_peak_wall"] < 1 and 0 < two["one_stream"]["frac_of_peak_wall"] < 1 and
                              0 < two["library_default"]["frac_of_peak_wall"] < 1 and 0 < two["synthesis_frac_of_peak_wall"] < 1), two
    ns = res["north_star_n48000"]
    assert ns["async_two_buffers"]["pipelined_calls"] >= 50 and ns["async_two_buffers"]["row_streams"] in ("ordinary", "by priority"), ns
    assert ns["async_two_buffers_one_stream"]["pipelined_calls"] == 0, ns
    assert 0 < ns["sync"]["frac_of_peak_wall"] < 1 and 0 < ns["sync_first_allocation"]["frac_of_peak_wall"] < 1 and ns["buffer_placement"]["first"]["placed"] is True, ns


def test_plain_bench_times_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) sets up, warms up, times the K steps and prints the line -- nothing beside the headline --
    and --dump-outputs writes the matrix of the last timed step: rows of it (a seeded sample, first and last included,
    under 64 MB) that the oracle, streamed through the same W + K calls of the same input, reproduces."""
    import numpy as np
    from oracle import oracle as O
    from sdft_amd.signals import sine_sweep
    n, m, warmup, steps = 8192, 1024, 1, 2
    res = run_bench(1, "--steps", str(steps), "--warmup", str(warmup), "--samples", str(n), "--dump-outputs", str(tmp_path / "dump"))
    assert res["steps"] == steps and res["warmup"] == warmup and res["full"] is False and res["ms_per_step"] > 0
    assert res["metric"].startswith("Msamples/s") and res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert abs(res["value"] - n / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * res["value"]
    for key in ("first_allocation", "analysis_plus_synthesis_msamples_s", "cpu_baseline", "extras", "configs"):
        assert key not in res, key
    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["dfts.npy", "dfts_rows.npy"], files
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in files) <= 64 << 20
    d, rows = np.load(tmp_path / "dump" / "dfts.npy"), np.load(tmp_path / "dump" / "dfts_rows.npy")
    assert d.dtype == np.float64 and rows.dtype == np.float64 and d.shape == (rows.size, m, 2) and rows.size < n
    idx = rows.astype(np.int64)
    assert idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) > 0)
    ref = O.best(m, "hann", 1.0, "f32f64")
    x = sine_sweep(n, channel=0, channels=1, dtype=np.float32)
    for _ in range(warmup + steps):                          # the plan is a stream: every call continues it
        want = ref.sdft(x)
    got = d[..., 0] + 1j * d[..., 1]
    assert np.abs(got - want[idx]).max() <= 1e-6 * np.abs(want[idx]).max()


def test_eight_rank_bench_plumbing():
    """The N = 8 branch of bench.py (configs[4]: channels sharded over 8 ranks, weak scaling) has never seen 8 GPUs; so that
    the first such run cannot fail on plumbing it runs here with 8 ranks -- nccl where 8 GPUs exist, else all ranks on the
    one GPU over gloo: 2 channels per rank, short calls, ONE JSON line, value = all ranks' samples / slowest rank's time."""
    import torch
    backend = {} if torch.cuda.device_count() >= 8 else {"SDFT_BENCH_BACKEND": "gloo"}
    res = run_bench(8, "--steps", "2", "--warmup", "1", "--samples", "4096", "--channels-per-gpu", "2", "--no-extras", "--full", env_extra=backend)
    assert res["n_gpus"] == 8 and res["config"]["channels_total"] == 16 and res["config"]["samples_per_channel"] == 4096
    assert res["scaling"] == "weak" and res["cpu_baseline"] is None
    assert abs(res["value"] - 16 * 4096 / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * res["value"]
    assert "configs[4]" in res["config"]["workload"] and "2/GPU" in res["config"]["workload"]
    assert res["ranks"]["ranks_in_collectives"] == 8 and res["ranks"]["world_size"] == 8
    # round 6: a rank whose arena (matrix + 64 GiB) does not fit -- eight ranks on one GPU here, a GPU somebody else is using on a real node --
    # takes its first allocation and the census says how many did, with the spread of the ranks' store-only rates and first-allocation fractions
    rk = res["ranks"]
    assert 0 <= rk["ranks_with_a_placed_matrix"] <= 8
    assert rk["placement_gbs_min_over_ranks"] <= rk["placement_gbs_max_over_ranks"]
    assert (rk["placement_gbs_min_over_ranks"] == 0) == (rk["ranks_with_a_placed_matrix"] < 8), rk
    assert 0 < rk["first_allocation_frac_min_over_ranks"] <= rk["first_allocation_frac_max_over_ranks"] < 1, rk
    assert res["first_allocation"]["value"] > 0 and res["buffer_placement"]["placed"] in (True, False)


def _hip_rank(rank, world, port, q):
    """One rank of a sharded job on the HIP path: its block of channels through a batched plan, digests all-reduced."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from sdft_amd import shard
    from sdft_amd.sdft import SDFT
    from sdft_amd.signals import sine_sweep
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(rank % torch.cuda.device_count())
        channels, n, m = 5, 3000, 64
        first, count = shard.channel_block(channels, world, rank)
        x = np.stack([sine_sweep(n, channel=c, channels=channels) for c in range(first, first + count)])
        with SDFT(m, "hann", 1.0, "f32f64", channels=count) as p:
            d = p.sdft(torch.from_numpy(x).cuda())
            y = p.isdft(d)
            local = float(d.real.sum().item())
            ysum = float(y.double().sum().item())
        shard.barrier()
        total = shard.sum_over_ranks(local)
        ytotal = shard.sum_over_ranks(ysum)
        q.put((rank, first, count, total, ytotal))
    finally:
        dist.destroy_process_group()


def test_two_rank_sharding_on_the_hip_path():
    """tests/test_shard_gloo.py covers the partition arithmetic with the oracle standing in for the device; here every rank
    runs its channel block through the HIP kernels (batched plan) and the all-reduced digests meet the oracle's."""
    import numpy as np
    import socket
    import torch.multiprocessing as mp
    from oracle import oracle as O
    from sdft_amd.signals import sine_sweep
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_hip_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want, ywant = 0.0, 0.0
    for c in range(5):
        ref = O.best(64, "hann", 1.0, "f32f64")
        d = ref.sdft(sine_sweep(3000, channel=c, channels=5))
        want += float(d.real.sum()); ywant += float(ref.isdft(d).astype(np.float64).sum())
    assert [(r[1], r[2]) for r in res] == [(0, 3), (3, 2)]
    assert all(np.isclose(r[3], want, rtol=1e-9, atol=1e-9) and np.isclose(r[4], ywant, rtol=1e-6, atol=1e-6) for r in res)
    assert res[0][3] == res[1][3]
