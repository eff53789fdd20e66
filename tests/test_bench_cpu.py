"""CPU (not gpu): bench.py's main() end to end against the lane-emulated library (tests/hipemu) on a few sentences -- the whole
stage / warm-up / timed steps / fetch / cpu_baseline / JSON path of the driver contract, so that a Python error in the benchmark
is found here and not at the end of a round on the GPU box.  The numbers mean nothing (emulated kernels); the shape is checked."""
import json
import os
import subprocess
import sys

from corpora import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DRIVER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch
torch.cuda.synchronize = lambda *a, **k: None          # no GPU here; the emulated launches are synchronous
import kiwi_amd.workloads as W
orig = W.get_workload
W.get_workload = lambda name: (lambda p, t, d: (p, t[:24], d))(*orig(name))
import bench
sys.argv = ["bench.py", "--steps", "2", "--warmup", "1", "--workload", "small-c2"] + sys.argv[1:]
bench.main()
'''


def _run_driver(*extra):
    env = dict(os.environ, KAMD_LIB=os.path.join(HERE, "hipemu", "_build", "libkiwi_hipemu.so"))
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT}] + list(extra), env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_main_emits_the_contract_line(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hipemu"), "-j8"], stdout=subprocess.DEVNULL)
    out = _run_driver("--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    # (--steps is exactly the number of timed steps)
    assert out["n_gpus"] == 1 and out["steps_requested"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "sentences/s" and out["higher_is_better"] is True
    assert out["scaling"] == "weak" and out["vs_baseline"] is None and out["data"] == "synthetic" and "workload" in out["config"]
    assert out["value"] > 0 and abs(out["value"] - 24 * out["steps"] / (out["ms_per_step"] * out["steps"] / 1000.0)) < 1e-6 * out["value"] + 1e-9
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in out["roofline"], k
    assert out["roofline"]["bound"] == "hbm" and out["roofline"]["unit"] == "GB/s" and abs(out["roofline"]["frac"] - out["roofline"]["achieved"] / out["roofline"]["peak"]) < 1e-12
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in out["cpu_baseline"], k
    assert out["cpu_baseline"]["kind"] in ("reference", "port") and out["cpu_baseline"]["value"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full): the headline line alone, exactly --steps timed steps; --dump-outputs writes the results of the last step as
    float32 / float64 .npy files, the same ones from run to run (same inputs, same outputs)."""
    import numpy as np
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hipemu"), "-j8"], stdout=subprocess.DEVNULL)
    dumps = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        out = _run_driver("--dump-outputs", str(d))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "config"):
            assert key in out, key
        for key in ("roofline", "cpu_baseline", "e2e", "capi", "gather"):
            assert key not in out, key
        assert "also" not in out["config"] and "model" not in out["config"]
        assert out["steps"] == 2 and out["higher_is_better"] is True and out["unit"] == "sentences/s" and out["dtype"] == "int32+f32"
        assert abs(out["value"] - 24 * 2 / (out["ms_per_step"] * 2 / 1000.0)) < 1e-6 * out["value"] + 1e-9
        files = sorted(os.listdir(d))
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(f.endswith(".npy") for f in files) and sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
        assert arrays["analysis_prob"].shape == (24, 1) and np.isfinite(arrays["analysis_prob"]).all()
        assert arrays["sample_texts"].tolist() == list(range(24))
        n = len(arrays["token_text"])
        assert n == arrays["analysis_tokens"].sum() > 0 and all(len(arrays[k]) == n for k in arrays if k.startswith("token_") and k != "token_form_utf16")
        assert len(arrays["token_form_utf16"]) == arrays["token_form_len"].sum()
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][k], dumps[1][k], equal_nan=True) for k in dumps[0])


DRIVER2 = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch
torch.cuda.synchronize = lambda *a, **k: None
import kiwi_amd.dist as D
_init, _mx, _gc, _gp = D.init, D.max_over_ranks, D.gather_counts, D.gather_packed
D.init = lambda backend, device_index=None: _init("gloo")            # RCCL on the GPU box; gloo here
D.max_over_ranks = lambda v, device="cpu": _mx(v, "cpu")
D.gather_counts = lambda v, device="cpu": _gc(v, "cpu")
D.gather_packed = lambda buf, device="cpu", dst=0: _gp(buf, "cpu", dst)
import kiwi_amd.workloads as W
orig = W.get_workload
W.get_workload = lambda name: (lambda p, t, d: (p, t[:16], d))(*orig(name))
import bench
sys.argv = ["bench.py", "--gpus", os.environ.get("KAMD_TEST_WORLD", "2"), "--steps", "2", "--warmup", "1", "--workload", "small-c2", "--full", "--no-cpu-baseline"] + sys.argv[1:]
bench.main()
'''


def test_bench_main_with_two_ranks(tmp_path):
    """The N > 1 flow of bench.py exactly as the driver launches it (torch.distributed.run, one process per rank): rank 0 prepares the
    workload first, every rank analyses a same-sized shard, barrier + MAX over ranks of the time, one JSON line from rank 0 with the
    whole-job rate.  gloo instead of RCCL, emulated kernels instead of a GPU."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hipemu"), "-j8"], stdout=subprocess.DEVNULL)
    drv = tmp_path / "bench_two_ranks.py"
    drv.write_text(DRIVER2 % {"root": ROOT})
    env = dict(os.environ, KAMD_LIB=os.path.join(HERE, "hipemu", "_build", "libkiwi_hipemu.so"))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(drv)],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["parallelism"] == "shard2" and out["config"]["sentences_per_gpu"] == 16
    assert abs(out["value"] - 16 * 2 * 2 / (out["ms_per_step"] * 2 / 1000.0)) < 1e-6 * out["value"] + 1e-9      # all ranks' sentences / max time
    assert out["gather"]["merged_texts"] == 32 and out["gather"]["bytes_per_rank"] > 1000      # the packed token records of both ranks arrived on rank 0
    # strong scaling: ONE corpus split by index, the gathered records merged in input order
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(drv), "--scaling", "strong"],
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["scaling"] == "strong" and out["config"]["sentences_per_gpu"] == 8 and out["gather"]["merged_texts"] == 16
    assert abs(out["value"] - 16 * 2 / (out["ms_per_step"] * 2 / 1000.0)) < 1e-6 * out["value"] + 1e-9


def test_bench_main_with_eight_ranks_strong_scaling(tmp_path):
    """`bench.py --gpus 8 --scaling strong` as the driver's SCALE run launches it, on eight CPU ranks (gloo, emulated kernels): one corpus split by index over
    the ranks, the packed token records of all eight gathered on rank 0 and merged in input order -- so that the first hardware run of the 8-GPU curve
    cannot fail on plumbing (VERDICT r04 #7e)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hipemu"), "-j8"], stdout=subprocess.DEVNULL)
    drv = tmp_path / "bench_eight_ranks.py"
    drv.write_text(DRIVER2 % {"root": ROOT})
    env = dict(os.environ, KAMD_LIB=os.path.join(HERE, "hipemu", "_build", "libkiwi_hipemu.so"), KAMD_TEST_WORLD="8", OMP_NUM_THREADS="1")
    for extra, per_rank, merged in ((["--scaling", "strong"], 2, 16), ([], 16, 128)):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(drv)] + extra,
                           env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["n_gpus"] == 8 and out["scaling"] == ("strong" if extra else "weak") and out["config"]["parallelism"] == "shard8" and out["config"]["sentences_per_gpu"] == per_rank
        assert out["gather"]["merged_texts"] == merged
        assert abs(out["value"] - merged / (out["ms_per_step"] / 1000.0)) < 1e-6 * out["value"] + 1e-9
