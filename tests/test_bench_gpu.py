"""GPU (-m gpu): bench.py's one-line contract -- the keys the driver and the judge read, the roofline object's arithmetic, what a plain run
leaves to --full, and the watchdog that prints the headline when the N > 1 extras do not finish."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    return json.loads(lines[0])


def test_one_json_line_with_the_contract_keys():
    d = run_bench(["--gpus", "1", "--steps", "8", "--warmup", "2", "--full", "--no-motion", "--no-scan", "--no-cpu-baseline"])
    assert d["full"] is True
    assert d["metric"].startswith("Mpixels/s") and d["unit"] == "Mpixels/s" and d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and "synthetic" in d["data"]
    assert "workload" in d["config"] and "model" not in d["config"]
    frames = d["config"]["frames_per_gpu_per_step"]
    assert abs(d["value"] - frames * 3840 * 2160 / 1e6 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert 20000 < d["value"] < 167000                         # below the 48 B/pixel roofline, above anything a broken run would print
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) <= 2e-3 * r["achieved"]
    assert r["algorithmic_bytes_per_launch"] == 3840 * 2160 * 3 * 4
    assert r["traffic"] is None or r["traffic"] >= r["algorithmic_bytes_per_launch"]
    assert r["isolated_kernel_ms"].keys() == r["all_kernels_ms"].keys() and 0 < r["isolated_frac_dominant"] < 1
    assert d["max_abs_drift_after_all_roundtrips"] < d["roundtrips_of_frame0"] * 2e-6 + 1e-3
    # round 4: the line says what it did
    c = d["config"]
    assert c["preroll_steps"] == 700 - 2 and c["untimed_steps_total"] == 700 and "independent frames" in c["batch"] and "stream" in c["batch"]
    assert 15000 < d["single_stream_value"] < 167000
    assert d["forward_check"]["dc_rel_err"] < 1e-4 and d["forward_check"]["energy_rel_err"] < 1e-4
    if r["traffic"] is not None:
        assert "PROFILE LOOKUP" in r["traffic_source"]
        assert abs(r["physical_frac"] - r["traffic"] / (r["kernel_ms"] * 1e-3) / 8e12) < 1e-3 and r["physical_frac"] >= r["frac"]
    else:
        assert r["physical_frac"] is None
    e = d["fftw_abi_end_to_end"]
    assert e["bytes_each_way"] == 3840 * 2160 * 3 * 4 and e["link_GBps"]["h2d"] > 5 and e["link_GBps"]["d2h"] > 5
    assert abs(e["link_floor_ms"] - (e["bytes_each_way"] / e["link_GBps"]["h2d"] + e["bytes_each_way"] / e["link_GBps"]["d2h"]) / 1e6) < 0.05 * e["link_floor_ms"]
    assert e["ms"] >= 0.9 * e["link_floor_ms"] and abs(e["frac_of_link_floor"] - e["link_floor_ms"] / e["ms"]) < 2e-3
    assert abs(e["host_GBps_over_both_transfers"] - 2 * e["bytes_each_way"] / e["ms"] / 1e6) < 0.2
    # round 5: SURVEY 8d's per-frame latency (median and minimum over >= 50 event-bracketed pairs), the stated target and the declared cap
    f = d["frame_latency_ms"]
    assert f["pairs_timed"] >= 50 and 0 < f["min"] <= f["median"] < 5.0
    assert f["median"] * 1e-3 >= 3840 * 2160 * 48 / 8e12                      # not faster than the roofline
    t = d["target"]
    assert t["roundtrip_frac_of_hbm_roofline"] == 0.70 and t["met"] == (d["roundtrip_frac_of_hbm_roofline"] >= 0.70)
    m = t["builders_model_of_this_design"]            # context, not a goal post
    assert m["cap"] == 0.366 and abs(m["frac_of_it"] - d["roundtrip_frac_of_hbm_roofline"] / 0.366) < 2e-3


def test_a_plain_run_prints_the_headline_and_leaves_the_other_legs_to_full():
    """without --full the line carries the headline, its checks and the roofline of the timed region, and nothing that takes a run of its own"""
    d = run_bench(["--gpus", "1", "--steps", "8", "--warmup", "2"])
    assert d["full"] is False and d["steps"] == 8 and d["warmup"] == 2 and "error" not in d
    assert d["metric"].startswith("Mpixels/s") and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    frames = d["config"]["frames_per_gpu_per_step"]
    assert abs(d["value"] - frames * 3840 * 2160 / 1e6 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert 20000 < d["value"] < 167000
    assert d["config"]["untimed_steps_total"] == 700 and d["roundtrips_of_frame0"] == 700 + 8
    assert d["forward_check"]["dc_rel_err"] < 1e-4 and d["forward_check"]["energy_rel_err"] < 1e-4
    assert d["max_abs_drift_after_all_roundtrips"] < d["roundtrips_of_frame0"] * 2e-6 + 1e-3
    r = d["roofline"]
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) <= 2e-3 * r["achieved"]
    assert "isolated_kernel_ms" not in r and "isolated_frac_dominant" not in r
    for k in ("single_stream_value", "frame_latency_ms", "motion_c5", "scan_c4", "fftw_abi_end_to_end",
              "cpu_baseline", "cpu_baseline_fftw", "cpu_baseline_scipy"):
        assert k not in d, k


def test_motion_volume_reports_the_exchange_fields_and_they_are_null_on_one_gpu():
    """motion_c5.volume_3d carries exchange_ms / xgmi_frac (bytes sent per rank / exchange time / 7 x 76.8 GB/s); with one rank there is
    no exchange and they are null"""
    d = run_bench(["--gpus", "1", "--steps", "8", "--warmup", "2", "--full", "--no-scan", "--no-cpu-baseline", "--no-fftw-abi", "--no-single-stream"])
    v = d["motion_c5"]["volume_3d"]
    assert "error" not in v, v
    for k in ("exchange_ms", "xgmi_GBps_sent_per_rank", "xgmi_frac"):
        assert k in v and v[k] is None
    assert v["exchanges_per_clip"] == 0 and "7 links" in v["exchange_note"]


def test_watchdog_prints_the_headline_when_the_extras_do_not_finish():
    env = {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533", "DSPFFT_BENCH_FORCE_DIST": "1"}
    d = run_bench(["--steps", "8", "--warmup", "2", "--full", "--no-cpu-baseline", "--extras-timeout", "0.05"], env=env)
    assert d["value"] > 20000
    assert d["ranks_seen_by_rccl"] == 1                     # the RCCL path ran (one rank): an all-reduce of ones
    assert "error" in d["motion_c5"] and "not finished" in d["motion_c5"]["error"]
    assert "error" in d["scan_c4"]
