"""bench.py as the driver runs it: one JSON line, the --gpus N launcher really starts N ranks, the reporting fields add up."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env,
                       timeout=timeout, cwd=ROOT)
    return p


def _json_line(p):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_launcher_refuses_more_ranks_than_gpus_without_share_gpu():
    # runs without a GPU too: the parent must fail loudly before any rank is started
    p = _run("--gpus", "64")
    assert p.returncode != 0 and "--gpus 64" in (p.stderr + p.stdout)


def test_gpus_flag_must_agree_with_the_launcher_environment():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                       env=env, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)


def test_rank_pinning_is_best_effort_and_never_raises():
    """bench.py pins each rank of an N > 1 run to the CPUs local to its GPU before its first GPU call (KFD topology -> DRM render
    node -> local_cpulist).  Without a GPU (this container), with unreadable nodes (the host's other GPUs inside a one-GPU box) or
    with an index past the visible GPUs it must report what happened and leave the affinity alone."""
    sys.path.insert(0, ROOT)
    import bench
    before = os.sched_getaffinity(0)
    for idx in (0, 99):
        info = bench.pin_to_gpu_numa_node(idx)
        assert set(info) >= {"gpu", "numa_node", "cpus_local", "cpus_used", "pinned"} and info["gpu"] == idx
        if not info["pinned"]:
            assert os.sched_getaffinity(0) == before
    os.sched_setaffinity(0, before)


@pytest.mark.gpu
def test_gpus_2_spawns_two_ranks_on_one_card():
    """`python bench.py --gpus 2` with no launcher: the parent spawns two fresh rank processes (here both on cuda:0, gloo for
    the collectives -- the RCCL/xGMI form needs two cards) and rank 0 reports the aggregate."""
    r = _json_line(_run("--gpus", "2", "--share-gpu", "--backend", "gloo", "--frames", "4096", "--bits", "1024",
                        "--steps", "3", "--warmup", "1", "--full"))
    assert r["n_gpus"] == 2 and r["scaling"] == "weak"
    assert r["ranks"]["world_size"] == 2 and r["ranks"]["ranks_in_blob_allreduce"] == 2
    assert r["ranks"]["blob_checksum_identical_on_all_ranks"] is True
    assert len(r["per_rank_Mbit_s"]) == 2 and all(v > 0 for v in r["per_rank_Mbit_s"])
    # every rank reports where it was pinned (both ranks share cuda:0 here: the same NUMA node) and its own clock under load
    pr = r["ranks"]["per_rank"]
    assert len(pr) == 2 and all(500 < x["clock_mhz_under_load"] < 3000 for x in pr)
    assert all(x["pinned_to_gpu_local_cpus"] and x["cpus"] >= 1 for x in pr), pr
    assert "cpu_baseline" not in r            # rank 0 at N=1 only
    assert 0 <= r["ber"] < 1e-2
    # the N > 1 line carries its own correctness evidence: every rank checked frames of ITS shard of the last timed launch against the
    # scalar reference (bytes and every decision word); flags and counts are summed over the ranks
    par = r["parity"]
    assert par["ranks_checked"] == 2 and par["ranks_bit_exact"] == 2 and par["bit_exact"] is True, par
    assert par["frames_checked"] == 128 and par["frames_per_rank"] == 64 and par["decision_words_bit_exact"] and par["chainback_bytes_bit_exact"], par
    assert r["ranks"]["backend"] == "gloo" and r["ranks"]["collective_library"]["name"] == "gloo"
    assert "configs" not in r                 # the other BASELINE configs ride on the default N = 1 line only


@pytest.mark.gpu
def test_single_rank_line_is_self_consistent():
    r = _json_line(_run("--frames", "8192", "--bits", "2048", "--steps", "4", "--warmup", "1", "--cpu-seconds", "2", "--full"))
    assert r["n_gpus"] == 1 and r["unit"] == "Mbit/s" and r["dtype"] == "u16" and r["vs_baseline"] is None
    bits = 8192 * 2048 * 4
    assert abs(r["value"] - bits / (r["ms_per_step"] * 4e-3) / 1e6) / r["value"] < 1e-6
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and rf["frac"] < 1
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (r["update_ms"] * 1e-3) / 1e9) < 1e-6 * rf["achieved"]
    e2e = r["roofline_end_to_end"]
    assert abs(e2e["achieved"] - e2e["bytes_per_info_bit"] * 8192 * 2048 / (r["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * e2e["achieved"]
    cb = r["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0
    if cb["kind"] == "reference":
        # threads really decode in parallel: the per-thread rate is within 2x of one thread alone
        assert cb["per_thread_Mbit_s"] * 2 > cb["simd_1thread_Mbit_s"]
    par = r["parity"]
    assert par["bit_exact"] and par["decision_words_bit_exact"] and par["chainback_bytes_bit_exact"]
    assert r["config"]["via"] == "pipeline" and "vit_hip_pipeline" in r["config"]["pipeline"]
    assert r["ms_per_step_min"] <= r["ms_per_step_median"] <= r["ms_per_step_max"]
    # the steady-state figure beside the wall-clock one: the same bits priced at the median step
    assert abs(r["value_steady"] - 8192 * 2048 / (r["ms_per_step_median"] * 1e-3) / 1e6) < 1e-6 * r["value_steady"]
    assert 500 < r["clock_mhz"]["before_warmup"] < 3000 and 500 < r["clock_mhz"]["after"] < 3000
    assert 500 < r["clock_mhz"]["under_load"] < 3000 and r["clock_mhz"]["under_load_probe"]["probe_ms"] < 30


@pytest.mark.gpu
def test_headline_line_carries_its_spread_and_both_routes_agree():
    """the default workload (BASELINE configs[1]) through the shipped pipeline API: the per-step times recorded on the device
    bracket their median, the median agrees with the wall-clock figure, and the Python re-implementation of the schedule
    (--via python) lands on the same rate."""
    a = _json_line(_run("--config", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--parity", "--full"))
    assert a["parity"]["bit_exact"] and a["parity"]["frames_checked_vs_scalar_reference"] == 512
    # the default workload's line also carries BASELINE configs[2], [3] (one GPU's share) and [4], each timed through the same pipeline
    # API with its own roofline and parity block (the reference runs its whole matrix in one invocation: run_benchmark.cpp:168-179)
    cfgs = a["configs"]
    assert [c["baseline_config"] for c in cfgs] == [0, 2, 3, 4] and not any("error" in c for c in cfgs), cfgs
    # configs[0]: the reference's first example, ONE 4096-bit frame through the drop-in's reset -> update -> chainback -- a latency
    # record (ns per trellis step), bit-exact incl. every decision word; the in-place kernel keeps it under 0.25 ms
    c0 = cfgs.pop(0)
    assert c0["config"]["frames_per_gpu"] == 1 and c0["config"]["bits_per_frame"] == 4096 and c0["config"]["via"] == "host"
    assert c0["parity"]["bit_exact"] and c0["parity"]["decision_words_bit_exact"] and 0 <= c0["ber"] < 1e-2
    assert c0["ms_per_step_median"] < 0.25 and 20 < c0["ns_per_trellis_step_update"] < 60, (c0["ms_per_step_median"], c0["ns_per_trellis_step_update"])
    for c, (K, dt, F, nchk) in zip(cfgs, ((9, "u16", 65536, 64), (7, "u8", 32768, 64), (15, "u16", 4096, 8))):
        assert f"K={K} " in c["config"]["workload"] and c["dtype"] == dt and c["config"]["frames_per_gpu"] == F
        assert c["parity"]["bit_exact"] and c["parity"]["frames_checked_vs_scalar_reference"] == nchk, c["parity"]
        assert c["value"] <= c["value_steady"] * 1.02 and c["value_sustained"] > 0.9 * c["value_steady"], c
        rf = c["roofline"]
        assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (c["update_ms"] * 1e-3) / 1e9) < 1e-6 * rf["achieved"] and 0 < rf["frac"] < 1
        assert rf["traffic"] is not None and 0.95 < rf["traffic"] / rf["algorithmic_bytes_per_launch"] < 1.15, rf
        assert 0.5 < c["roofline_valu"]["frac"] < 1.05 and 0 <= c["ber"] < 1e-2, c
    assert cfgs[1]["update_launches_in_flight"] == 2
    assert sum(c["seconds_spent"] for c in cfgs) + c0["seconds_spent"] < 90, [c["seconds_spent"] for c in cfgs]
    assert a["config"]["frames_per_gpu"] == 65536 and a["config"]["bits_per_frame"] == 8192 and a["config"]["via"] == "pipeline"
    assert a["ms_per_step_min"] <= a["ms_per_step_median"] <= a["ms_per_step_max"]
    # wall clock over the timed region = the steady step (the median) + one pipeline fill and drain (the first update has no
    # chainback beside it, the last chainback no update: about one millisecond over the 20 steps) + the first steps' run-in
    # (bounds with room for ONE slow step among the twenty: a fresh box's first run showed 3.64 ms against a 3.30 ms median once)
    assert abs(a["ms_per_step_median"] - a["ms_per_step"]) / a["ms_per_step"] < 0.15, a
    assert a["value"] <= a["value_steady"] * 1.01 and a["value_steady"] < a["value"] * 1.18, (a["value"], a["value_steady"])
    # the vector-issue roofline is priced against the rate measured on the card; the guide's nominal 2 clocks per instruction
    # is quoted beside it and is the larger of the two
    rv = a["roofline_valu"]
    assert rv["peak_spec"] > rv["peak"] and 0 < rv["frac_of_spec"] < rv["frac"] < 1.0, rv
    assert len(a["ms_per_step_series"]) == 20 and abs(sum(a["ms_per_step_series"]) / 20 - a["ms_per_step"]) < 0.05 * a["ms_per_step"]
    b = _json_line(_run("--config", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--via", "python", "--full"))
    assert "configs" not in b
    assert b["config"]["via"] == "python"
    # the Python re-implementation queues the same kernels from the interpreter (a few microseconds later per launch): it may
    # trail the C route by a few per cent, never lead it by much
    assert -0.03 < (a["value"] - b["value"]) / b["value"] < 0.08, (a["value"], b["value"])


@pytest.mark.gpu
def test_config_presets_name_the_baseline_configs():
    """--config 3 is one GPU's share of the 8-GPU hard-decision run; the small-batch schedule (two updates in flight) serves it"""
    r = _json_line(_run("--config", "3", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--full"))
    assert r["dtype"] == "u8" and r["config"]["frames_per_gpu"] == 32768 and r["config"]["bits_per_frame"] == 8192
    assert "HARD8" in r["config"]["workload"]
    assert r["update_launches_in_flight"] == 2 and r["roofline"]["launches_in_flight"] == 2
    assert 0 < r["ber"] < 1e-2


@pytest.mark.gpu
def test_plain_line_is_the_headline_only_and_dumps_repeatable_outputs(tmp_path):
    """without --full the line carries the headline and nothing that needs runs of its own; --dump-outputs writes the decoded
    bytes of the last timed step, the same on every run with the same arguments"""
    import numpy as np

    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = _json_line(_run("--frames", "4096", "--bits", "2048", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in r, key
        assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Mbit/s" and r["higher_is_better"] is True and r["dtype"] == "u16"
        assert abs(r["value"] - 4096 * 2048 * 3 / (r["ms_per_step"] * 3e-3) / 1e6) / r["value"] < 1e-6
        assert len(r["ms_per_step_series"]) == 3
        assert not {"configs", "cpu_baseline", "parity"} & set(r) and r["sustained"] is None and r["ber"] is None
        got = np.load(d / "decoded_bytes.npy")
        assert got.dtype == np.float32 and got.shape == (4096, 2048 // 8)
        assert np.array_equal(np.load(d / "decoded_frame_index.npy"), np.arange(4096))
        dumps.append(got)
    assert np.array_equal(dumps[0], dumps[1])
