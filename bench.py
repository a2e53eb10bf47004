#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's config, on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload NAME] [--scaling weak|strong] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the outputs when --dump-outputs is given and prints the line.
Everything else the script measures runs only with --full (off by default): the live PMC passes, the HIP-event loop and
the copy ceiling of `roofline`, the objects `strong_config5`, `configs`, `rfft_reference_bench`, `cpu_baseline` and
`vendor_rocfft`, and under --scaling strong the end-to-end and per-slab-kernel legs and the model.  The --no-* switches
narrow a --full run.

--dump-outputs DIR writes what the last timed step computed -- the `out` tensor a caller of the timed path receives, in
the run's precision -- as DIR/out.npy; above DUMP_BYTES it is a fixed, seeded sample (dump_sample).  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.

A "step" is one pass of the hot path (one plan_fft'd `fft(out, x)` call) over one batch of synthetic complex64 input
that is already resident in HBM.  At N=1 the workload is BASELINE.json configs[1]: 100k x 1024 1-D C2C fp32 with the
user radix list [2] ("radix-2 Stockham").

Multi-GPU: one process per GPU.  Started WITHOUT a launcher (`python bench.py --gpus N`, WORLD_SIZE unset) this
process spawns the N ranks itself -- before torch or HIP is touched, each rank a fresh child process -- and relays rank
0's JSON line; started under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` it is one of
the ranks.  Either way WORLD_SIZE must equal --gpus, and `ranks_seen` (an all-reduce of ones over RCCL) is printed.
  --scaling weak   (default) every rank owns its own 100k x 1024 slab, no data-path collective: value = rows of all
                   ranks * FLOPs / max-over-ranks time
  --scaling strong BASELINE configs[4]: ONE 10 x 128^3 batch split over the ranks (2,2,1,..,1 volumes at N=8: the ideal
                   speed-up is 5x, 3.33x at N=4, 2x at N=2); "compute, shards resident" and "end-to-end incl. the
                   scatter/gather of ShardedFFT.fft_from_root over RCCL" are reported separately
A --full run of the headline also carries the strong-scaling leg as the object `strong_config5`.

Prints ONE JSON line (rank 0): `metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, `config`, and
  roofline       HBM roofline of the dominant kernel; `achieved` / `frac` = algorithmic bytes per launch (16 B per complex
                 element: one 8-B read + one 8-B write) / ms_per_step of the K TIMED STEPS; `traffic` =
                 HBM bytes per step from the committed profile of the same command.  With --full: the same figure from
                 HIP events on the launch stream inside libmifft (mifft_time_exec, a separate loop right after the timed
                 steps) is `frac_hip_events`; `traffic` comes from `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`
                 child passes of this command, run by this process BEFORE it touches the GPU (N=1 headline run); `copy`
                 = COPY kernels with the tile shapes and cache policy of the FFT passes moving the same bytes in this
                 run on this box (tools/libmifft_probe.so: what the chip gives a kernel that only moves the pass's bytes)
  ramp           the untimed clock / cache ramp that precedes the W warm-up steps (ms, execs)
Extra objects (--full):
  configs        (N=1) the other four BASELINE.json configs, each timed the same way in this run
  rfft_reference_bench  (N=1) the shapes of the reference's own GPU benchmark in ITS mode: real input, full complex
                 spectrum out (fft/bench.mojo:57-97,108-124); fraction of the roofline on 4 B read + 8 B written per point
  cpu_baseline   (N=1) the CPU oracle (restatement of the reference's multi-threaded CPU path) on this host's cores on a
                 bounded sample of the workload, with its 1-thread figure and the SciPy / NumPy comparators of the
                 reference's benchmark-cpu-others/benchmark.py beside it
  vendor_rocfft  (N=1, when tools/vendor_fft_bench is built) bench-only comparator column: rocFFT on the five BASELINE
                 shapes, in its own process (the analogue of the reference's cuFFT harness); never part of libmifft
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"
METRIC = "C2C GFLOP/s (5Nlog2N) + ms/transform, 100k×1024 fp32 @1/2/4/8 MI355X"

WORKLOADS = {
    # name: (shape without the complex dim, user bases, BASELINE.json config index)
    "1d_100kx1024_radix2": ((100000, 1024), [[2]], 1),
    "1d_500kx93_radix31x3": ((500000, 93), [[31, 3]], 2),
    "1d_500kx128": ((500000, 128), None, 0),
    "2d_100x640x480": ((100, 640, 480), None, 3),
    "3d_10x128x128x128": ((10, 128, 128, 128), None, 4),
    # further shapes of the reference's own bench / README tables (not BASELINE configs; index -1)
    "3d_100x64x64x64": ((100, 64, 64, 64), None, -1),
    "3d_1x256x256x256": ((1, 256, 256, 256), None, -1),
    "1d_100x16384": ((100, 16384), None, -1),
    "2d_10x1920x1080": ((10, 1920, 1080), None, -1),
    "2d_1x3840x2160": ((1, 3840, 2160), None, -1),
    "2d_1x7680x4320": ((1, 7680, 4320), None, -1),
    "1d_64x1048576_fourstep": ((64, 1 << 20), None, -1),
    # lengths without a precompiled kernel: the tile kernel specialised at plan creation (hipRTC)
    "1d_290kx343_radix7": ((290000, 343), None, -1),
    "1d_330kx97_prime": ((330000, 97), None, -1),
    "2d_3200x100x100_plane": ((3200, 100, 100), None, -1),
    # real input -> full complex spectrum (the reference's own benchmark mode, fft/bench.mojo:57-97): for profiling
    "1d_100kx1024_real": ((100000, 1024), [[2]], -1),
    "2d_100x640x480_real": ((100, 640, 480), None, -1),
    "3d_10x128x128x128_real": ((10, 128, 128, 128), None, -1),
}
DEFAULT_WORKLOAD = "1d_100kx1024_radix2"
STRONG_WORKLOAD = "3d_10x128x128x128"
# the BASELINE.json configs other than the headline, in index order (the `configs` array of the N=1 line)
OTHER_BASELINE_CONFIGS = ["1d_500kx128", "1d_500kx93_radix31x3", "2d_100x640x480", "3d_10x128x128x128"]
# the shapes the reference's own GPU benchmark runs, which is the REAL-input one (bench_gpu_radix_n_rfft,
# fft/bench.mojo:57-97, shape list :108-124): real in, full complex spectrum out (`rfft_reference_bench` of the N=1 line)
RFFT_REFERENCE_SHAPES = [(250000, 93), (250000, 128), (100000, 1024), (100, 640, 480), (100, 64, 64, 64),
                         (10, 128, 128, 128), (1, 256, 256, 256)]
RAMP_S = float(os.environ.get("MIFFT_BENCH_RAMP_S", "0.05"))  # (the env override is for tools/ramp_probe.sh only)
DUMP_BYTES = 48 << 20  # --dump-outputs: at most this many bytes of samples (64 MB in all with room to spare)


def flops_5nlogn(shape):
    n = 1
    for d in shape[1:]:
        n *= d
    return 5.0 * n * math.log2(n) * shape[0]


def host_cpu_share(nproc):
    """Cores this process may really use: min(affinity, cgroup cpu.max quota, nproc)."""
    n = nproc
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def measured_traffic(workload, kernels):
    """HBM bytes per launch from the committed PMC passes (profiles/rNN_<workload>.json, written by
    tools/summarize_prof.py from `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs of THIS command,
    FETCH_SIZE corrected by the calibrated gfx950 factor); the newest profile whose kernel set matches the
    kernels of this run.  None otherwise -- counters cannot be collected from inside an un-profiled run."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{workload}.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        ks = [k for k in d.get("kernels", []) if "hbm_traffic_bytes" in k]
        names = " ".join(k["kernel"] for k in ks)
        if ks and len(ks) == len(set(kernels)) and (d.get("bench_kernels") in (None, sorted(set(kernels)))):
            best = (sum(k["hbm_traffic_bytes"] for k in ks), os.path.basename(f), names)
    return best


def dump_sample(shape, elem_bytes):
    """Which part of an output of `shape` (complex dim last) --dump-outputs writes: (lead, idx).  The output is viewed
    as slices along its `lead` leading dimensions -- whole transforms (lead = 1) when one fits DUMP_BYTES, else the
    slices of the next dimension, and so on -- and idx is a fixed seeded choice of as many slices as fit, ascending (all
    of them when the whole output fits).  It depends on the shape and element size only, so every run with the same
    arguments writes the same elements."""
    import numpy as np
    total = elem_bytes
    for d in shape:
        total *= d
    units = 1
    for lead in range(1, len(shape)):
        units *= shape[lead - 1]
        if total // units <= DUMP_BYTES:
            break
    k = min(units, DUMP_BYTES // (total // units))
    if k == units:
        return lead, np.arange(units)
    return lead, np.sort(np.random.default_rng(0).choice(units, size=k, replace=False))


def dump_outputs(dump_dir, out):
    """DIR/out.npy: the tensor the last timed step wrote (float32 or float64, like the run), or its dump_sample: an
    array (slices, *slice shape)."""
    import numpy as np
    import torch
    shape = tuple(out.shape)
    lead, idx = dump_sample(shape, out.element_size())
    view = out.reshape((-1,) + shape[lead:])
    sample = view if len(idx) == view.shape[0] else view[torch.as_tensor(idx, device=out.device)]
    arr = sample.cpu().numpy()
    os.makedirs(dump_dir, exist_ok=True)
    path = os.path.join(dump_dir, "out.npy")
    np.save(path, arr)
    sys.stderr.write(f"bench.py: {path}: {len(idx)} of {view.shape[0]} slices of out{list(shape)}, {arr.nbytes} bytes\n")


# ------------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N=1): the oracle port + the comparators of benchmark-cpu-others/benchmark.py:41-49
# ------------------------------------------------------------------------------------------------
def cpu_baseline(shape, bases, budget_s=12.0):
    """Oracle timed on a bounded sample (leading-batch subset) of the workload: all host threads (the `value`),
    one thread (the reference README's single-thread table, README.md:98-115), and beside them
    scipy.fft.fftn(workers=-1) and numpy.fft.fftn on complex64 like the reference's competitor harness."""
    import numpy as np
    from oracle import mifft_oracle as O

    cores = host_cpu_share(O.num_procs())
    rng = np.random.default_rng(1234)
    per = int(np.prod(shape[1:]))

    def run(b, workers):
        x = rng.standard_normal((b,) + tuple(shape[1:]) + (2,), dtype=np.float32)
        out = np.empty_like(x)
        plan = O.plan_fft(np.float32, np.float32, x.shape, x.shape, bases=bases, default_target="gpu")
        O.fft(out, x, plan=plan, cpu_workers=workers)  # warm-up (page faults, thread pool)
        t = time.perf_counter()
        O.fft(out, x, plan=plan, cpu_workers=workers)
        return time.perf_counter() - t

    def gflops(b, t):
        return flops_5nlogn((b,) + tuple(shape[1:])) / t / 1e9

    b0 = max(1, min(shape[0], (1 << 21) // per))
    t0 = max(run(b0, cores), 1e-4)
    b1 = int(max(b0, min(shape[0], b0 * (budget_s / 3) / t0, (1 << 28) // per)))
    t1 = run(b1, cores) if b1 > b0 else t0
    res = {
        "value": round(gflops(b1, t1), 3), "unit": "GFLOP/s", "cores": cores, "kind": "port",
        "sample": f"{b1} of {shape[0]} leading-batch entries of the same shape, all {cores} host threads, "
                  f"oracle/libmifft_oracle.so (C++ restatement of the reference CPU path; g++ -O3 -march=x86-64-v3 "
                  f"-ffp-contract=off -fopenmp), nproc={os.cpu_count()}, {t1 * 1e3:.1f} ms",
        "ms_per_transform": round(t1 * 1e3 / b1, 6),
    }
    # one thread (README.md:102-110): a sample sized to about a sixth of the budget
    bs = int(max(1, min(b1, b1 * (budget_s / 6) / max(t1 * cores, 1e-4))))
    ts = run(bs, 1)
    res["port_1thread"] = {"value": round(gflops(bs, ts), 3), "unit": "GFLOP/s", "cores": 1,
                           "sample": f"{bs} entries, {ts * 1e3:.1f} ms"}
    # comparators (benchmark-cpu-others/benchmark.py:35,41-49): complex64, axes = all but the batch
    try:
        import scipy.fft
        bc = int(max(1, min(b1, (1 << 25) // per)))
        data = (rng.standard_normal((bc,) + tuple(shape[1:]), dtype=np.float32)
                + 1j * rng.standard_normal((bc,) + tuple(shape[1:]), dtype=np.float32)).astype(np.complex64)
        axes = tuple(range(1, len(shape)))
        repeats = 2 if data.size > 2e7 else 5

        def avg(fn):
            fn()  # warm-up
            t = time.perf_counter()
            for _ in range(repeats):
                fn()
            return (time.perf_counter() - t) / repeats

        tsp = avg(lambda: scipy.fft.fftn(data, axes=axes, workers=cores))
        res["scipy_fftn"] = {"value": round(gflops(bc, tsp), 3), "unit": "GFLOP/s", "cores": cores,
                             "sample": f"scipy.fft.fftn(workers={cores}) (pocketfft), complex64, {bc} entries, "
                                       f"{repeats} repeats, {tsp * 1e3:.1f} ms"}
        bn = int(max(1, bc // 4))
        tnp = avg(lambda: np.fft.fftn(data[:bn], axes=axes))
        res["numpy_fftn"] = {"value": round(gflops(bn, tnp), 3), "unit": "GFLOP/s", "cores": 1,
                             "sample": f"numpy.fft.fftn, complex64 in (computes in complex128), {bn} entries, "
                                       f"{repeats} repeats, {tnp * 1e3:.1f} ms"}
    except Exception as e:  # a missing comparator must not cost the bench line
        res["comparators_error"] = repr(e)
    return res


_PROBE = None


def probe_lib():
    """tools/libmifft_probe.so (copy kernels, measurement tooling); None when it is not built."""
    global _PROBE
    if _PROBE is None:
        import ctypes
        path = os.path.join(ROOT, "tools", "libmifft_probe.so")
        if not os.path.exists(path):
            _PROBE = False
        else:
            L = ctypes.CDLL(path)
            L.probe_copy_flat.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
            L.probe_copy_cols.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_float)]
            L.probe_copy_pair.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
            _PROBE = L
    return _PROBE or None


def copy_ceiling(name, kernels, x, out, iters=30):
    """COPY kernels shaped like the passes of workload `name` (complex64 only), timed with HIP events on the current
    stream right after the FFT's timed steps: [{pass, ms}] or None.  1-D rows: one flat out-of-place copy with the cache
    policy of the selected kernel (`_nt` loads + stores, `_nts` stores, `_ntl` loads non-temporal).  100 x 640 x 480: the
    row pass as a flat copy x -> out with non-temporal loads + 16-column x 640-row tiles in place on `out`.  10 x 128^3:
    the plane pass as a flat copy with the plane kernel's 136 KB of LDS reserved (one workgroup per CU, one LDS round trip)
    + 32-column x 128-row tiles in place."""
    import ctypes
    L = probe_lib()
    if L is None or x.dtype != out.dtype or x.shape != out.shape or x.element_size() != 4:
        return None
    shape = WORKLOADS[name][0]
    n = 1
    for d in shape:
        n *= d
    ms = ctypes.c_float()

    def flat(nt, lds=0, wg=8):
        rc = L.probe_copy_flat(x.data_ptr(), out.data_ptr(), n, nt, lds, wg, iters, None, ctypes.byref(ms))
        return round(ms.value, 5) if rc == 0 else None

    def cols(outer, npts, inner, w, wg):
        rc = L.probe_copy_cols(out.data_ptr(), out.data_ptr(), outer, npts, inner, w, wg, iters, None, ctypes.byref(ms))
        return round(ms.value, 5) if rc == 0 else None

    def pair(nt1, lds1, wg1, outer, npts, inner, w, wg2):
        rc = L.probe_copy_pair(x.data_ptr(), out.data_ptr(), n, nt1, lds1, wg1, outer, npts, inner, w, wg2, iters, None,
                               ctypes.byref(ms))
        return round(ms.value, 5) if rc == 0 else None

    passes = []
    if len(shape) == 2:
        k = kernels[0]
        nt = 3 if k.endswith("_nt") else 2 if k.endswith("_nts") else 1 if k.endswith("_ntl") else 0
        passes.append({"pass": f"flat copy x -> out, nt={nt} ({k})", "ms": flat(nt)})
    elif name == "2d_100x640x480":
        passes.append({"pass": "rows480 as a flat copy x -> out, non-temporal loads", "ms": flat(1)})
        passes.append({"pass": "cols640: 16-column x 640-row tiles in place on out, 80 KB of LDS, one LDS round trip",
                       "ms": cols(shape[0], 640, 480, 16, 1)})
        passes.append({"pass": "PAIR: the two copies above alternating like the transform's passes (ms per pair)",
                       "ms": pair(1, 0, 8, shape[0], 640, 480, 16, 1), "pair": True})
    elif name == "3d_10x128x128x128":
        passes.append({"pass": "plane128x128 as a flat copy x -> out, 136 KB of LDS reserved (1 workgroup per CU), one "
                               "LDS round trip", "ms": flat(0, 136 * 1024 + 1024, 1)})
        passes.append({"pass": "cols128: 32-column x 128-row tiles in place on out, 32 KB of LDS",
                       "ms": cols(shape[0], 128, 128 * 128, 32, 4)})
        passes.append({"pass": "PAIR: the two copies above alternating like the transform's passes (ms per pair)",
                       "ms": pair(0, 136 * 1024 + 1024, 1, shape[0], 128, 128 * 128, 32, 4), "pair": True})
    else:
        return None
    if any(p["ms"] is None for p in passes):
        return None
    return passes


def vendor_compare(timeout_s=240):
    """Bench-only comparator column: rocFFT on the five BASELINE shapes through
    tools/vendor_fft_bench, a separate executable in its own process (the analogue of
    cufft-benchmark-main/cufft_benchmark.cu).  libmifft never links or calls a vendor FFT."""
    exe = os.path.join(ROOT, "tools", "vendor_fft_bench")
    if not os.path.exists(exe):
        return {"error": "tools/vendor_fft_bench not built (make -C tools)"}
    shapes = ["x".join(str(d) for d in WORKLOADS[w][0]) for w in ["1d_500kx128", DEFAULT_WORKLOAD] + OTHER_BASELINE_CONFIGS[1:]]
    try:
        r = subprocess.run([exe, "--iters", "50"] + shapes, capture_output=True, text=True, timeout=timeout_s)
    except Exception as e:
        return {"error": repr(e)}
    rows = []
    for line in r.stdout.splitlines():
        try:
            rows.append(json.loads(line))
        except Exception:
            pass
    out = {"library": "rocFFT (ROCm 7.2), own process, out of place C2C fp32, HIP events over 50 back-to-back execs",
           "rows": rows}
    if r.returncode:
        out["error"] = (r.stderr or "")[-300:]
    return out


# ------------------------------------------------------------------------------------------------
# live HBM-traffic counters: separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of THIS command
# ------------------------------------------------------------------------------------------------
FETCH_FACTOR = 2.0  # gfx950 counts the 8- / 16-byte-per-lane streaming reads of these kernels at 1/2 (guide, "HBM";
                    # calibrated 1.99993-2.00000 on a known-bytes copy of the same access shape in every profiles/rNN_*)


def live_pmc_traffic(workload, timeout_s=60):
    """{kernel name fragment: bytes per launch} measured NOW: two child runs of this script under rocprofv3 (one counter
    per pass: FETCH_SIZE and WRITE_SIZE do not fit one pass), started before this process has touched the GPU.  The
    program after `--` is python3 itself (no shell, no env hop).  None when rocprofv3 is missing or a pass fails -- the
    caller then falls back to the committed profile."""
    import csv
    import glob
    import shutil
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    res = {}
    tmp = tempfile.mkdtemp(prefix="mifft_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [prof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--workload", workload, "--steps", "5", "--warmup", "2", "--no-cpu-baseline",
                   "--no-configs", "--no-strong-leg", "--no-compare-vendor", "--no-live-pmc", "--no-copy-ceiling"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            if r.returncode:
                return None
            acc = {}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") == counter and "mifft::" in row["Kernel_Name"]:
                        acc.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
            if not acc:
                return None
            for k, v in acc.items():
                kib = sum(v) / len(v)
                res.setdefault(k, {})[counter] = kib * 1024.0 * (FETCH_FACTOR if counter == "FETCH_SIZE" else 1.0)
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {k: v["FETCH_SIZE"] + v["WRITE_SIZE"] for k, v in res.items() if len(v) == 2}
    return out or None


def _claim_stdout():
    """Keep stdout clean for the ONE JSON line: native libraries (RCCL prints a version banner on
    init) write to fd 1 directly, so fd 1 is pointed at stderr and the JSON goes to the saved fd."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    return os.fdopen(saved, "w")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/out.npy (a seeded sample above 48 MB)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline as well (module docstring); the --no-* switches below "
                         "narrow it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the array of the other BASELINE configs (N=1)")
    ap.add_argument("--no-strong-leg", action="store_true", help="skip the config-5 strong-scaling object")
    ap.add_argument("--compare-vendor", dest="vendor", action="store_true", default=None,
                    help="rocFFT comparator column in a --full run (default: on at N=1 for the headline workload)")
    ap.add_argument("--no-compare-vendor", dest="vendor", action="store_false")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not collect roofline.traffic with rocprofv3 child runs (N=1, headline workload only); the "
                         "committed profile is used instead")
    ap.add_argument("--no-copy-ceiling", action="store_true",
                    help="skip roofline.copy (copy kernels with the passes' tile shapes, tools/libmifft_probe.so)")
    ap.add_argument("--faithful", action="store_true", help="force the literal stage-per-pass kernel family")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"], help="arithmetic type (BASELINE metric: f32)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="N ranks share the visible GPU(s) and talk over gloo: exercises the N-rank launch, split and "
                         "timing code on a 1-GPU box (RCCL refuses two ranks on one device); not a scaling measurement")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` with no WORLD_SIZE -> N fresh rank processes
# ------------------------------------------------------------------------------------------------
def spawn_ranks(args, json_out):
    """Runs BEFORE anything touches the GPU in this process (no torch import, no HIP call): every rank is a new
    child process started with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, as torch.distributed.run would."""
    n = args.gpus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr, text=True))
    out0, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    line = None
    for ln in (out0 or "").splitlines():
        if ln.startswith("{"):
            line = ln
    if line:
        json_out.write(line + "\n")
        json_out.flush()
    bad = [rc for rc in rcs if rc]
    if bad or not line:
        sys.stderr.write(f"bench.py: rank exit codes {rcs}\n")
        return bad[0] if bad else 1
    return 0


class Bench:
    """One rank's state: device, process group, timing helpers."""

    def __init__(self, args):
        import torch

        import hackathon_fft_amd as mf
        self.torch, self.mf, self.args = torch, mf, args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={self.world}: start it as "
                             f"`python bench.py --gpus N` (it spawns the ranks) or under torch.distributed.run with "
                             f"--nproc-per-node equal to --gpus")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device: libmifft has no CPU path")
        ndev = torch.cuda.device_count()
        self.rehearse = bool(args.rehearse_on_one_gpu)
        self.dev_index = self.local_rank % ndev if self.rehearse else self.local_rank
        if self.dev_index >= ndev:
            raise SystemExit(f"bench.py: rank {self.rank} wants device {self.dev_index}, {ndev} visible")
        torch.cuda.set_device(self.dev_index)
        self.dev = torch.device("cuda", self.dev_index)
        # MIFFT_BENCH_FORCE_DIST=1 runs the RCCL code path even with one rank (1-GPU rehearsal of the N>1 launch)
        self.distributed = self.world > 1 or os.environ.get("MIFFT_BENCH_FORCE_DIST") == "1"
        self.dist = None
        self.ranks_seen = 1
        if self.distributed:
            import torch.distributed as dist
            self.dist = dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            if self.rehearse:
                dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
            else:
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev)
            one = torch.ones(1, device="cpu" if self.rehearse else self.dev)
            dist.all_reduce(one)
            self.ranks_seen = int(one.item())
            if self.ranks_seen != self.world:
                raise SystemExit(f"bench.py: all-reduce saw {self.ranks_seen} ranks, expected {self.world}")
        self.tdt = torch.float32 if args.dtype == "f32" else torch.float64
        self.esz = 4 if args.dtype == "f32" else 8
        self.ctx = mf.DeviceContext(self.dev_index)

    def barrier(self):
        self.torch.cuda.synchronize()
        if self.distributed:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def allmax(self, v):
        if not self.distributed:
            return v
        t = self.torch.tensor([v], device="cpu" if self.rehearse else self.dev, dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def timed(self, fn, steps, warmup):
        """ramp (>= RAMP_S of back-to-back calls, untimed) + `warmup` untimed calls + EXACTLY `steps` timed calls
        between barrier + synchronize on both sides; returns (max-over-ranks seconds, ramp calls, ramp seconds)."""
        torch = self.torch
        n_ramp = 0
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < RAMP_S:
            for _ in range(10):
                fn()
            n_ramp += 10
            torch.cuda.synchronize()
        ramp_s = time.perf_counter() - t_ramp
        for _ in range(warmup):
            fn()
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        self.barrier()
        return self.allmax(time.perf_counter() - t0), n_ramp, ramp_s

    def make_input(self, shape, seed_offset=0, comps=2):
        torch = self.torch
        gen = torch.Generator(device=self.dev).manual_seed(1234 + self.rank + seed_offset)
        x = torch.randn(tuple(shape) + (comps,), generator=gen, device=self.dev, dtype=self.tdt)
        return x, torch.empty(tuple(shape) + (2,), device=self.dev, dtype=self.tdt)

    def run_workload(self, name, steps, warmup, plan=None, x=None, out=None, dump_dir=None):
        """time one workload on this rank's GPU (every rank its own copy of the shape); rank 0 writes `out` as the last
        timed step left it to dump_dir when one is given"""
        mf = self.mf
        full = self.args.full
        shape, bases, cfg_idx = WORKLOADS[name]
        comps = 1 if name.endswith("_real") else 2
        if x is None:
            x, out = self.make_input(shape, comps=comps)
        if plan is None:
            plan = mf.plan_fft(self.tdt, self.tdt, x.shape, out.shape, bases=bases, ctx=self.ctx,
                               faithful_stages=self.args.faithful)
        elapsed, n_ramp, ramp_s = self.timed(lambda: mf.fft(out, x, self.ctx, plan=plan), steps, warmup)
        if dump_dir and self.rank == 0:
            dump_outputs(dump_dir, out)
        # kernel-level time: HIP events on the launch stream, inside the library
        launch_ms = mf.time_fft(out, x, plan=plan, iters=max(10, min(steps, 200)), ctx=self.ctx) if full else None
        ms_per_step = elapsed * 1e3 / steps
        elems = 1
        for d in shape:
            elems *= d
        # one complex (or real) read + one complex write per element, per exec on ONE gpu
        algo_bytes = (2.0 + comps) * self.esz * elems
        achieved = algo_bytes / (ms_per_step * 1e-3) / 1e9          # the K timed steps
        kernels = [plan.kernel_name(d) for d in range(len(shape) - 1)]
        copy = None
        if full and comps == 2 and self.args.dtype == "f32" and not self.args.no_copy_ceiling:
            passes = copy_ceiling(name, kernels, x, out)
            if passes:
                # two-pass shapes: the alternating pair is the ceiling (what pass 2 finds in the caches depends on pass 1)
                pairs = [p["ms"] for p in passes if p.get("pair")]
                cms = pairs[0] if pairs else sum(p["ms"] for p in passes)
                copy = {"ms": round(cms, 5), "frac": round(algo_bytes / (cms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "fft_over_copy": round(ms_per_step / cms, 4), "passes": passes,
                        "what": "copy kernels with the passes' tile shapes and cache policy (tools/copy_probe.hip), HIP "
                                "events over 30 launches each, same process, right after the timed steps"}
                # the copies overwrote `out`: leave the tensors as a transform left them
                mf.fft(out, x, self.ctx, plan=plan)
        traffic = measured_traffic(name, kernels)
        live = getattr(self, "live_traffic", {}).get(name)
        if live and len(live) == len(set(kernels)):
            # measured in THIS run: sum over the kernels of one step (one entry per distinct kernel)
            traffic = (sum(live.values()),
                       "live rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE child passes of this command in this run "
                       f"(FETCH_SIZE x {FETCH_FACTOR}, guide 'HBM'); committed: " + (traffic[1] if traffic else "none"), "")
        return {
            "workload": name, "baseline_config_index": cfg_idx, "shape": list(shape) + [comps],
            "ms_per_step": round(ms_per_step, 5),
            "gflops": round(flops_5nlogn(shape) / (ms_per_step * 1e-3) / 1e9, 2),
            "bases": bases if bases is not None else "reference gpu default",
            "stages": [plan.stages(d) for d in range(len(shape) - 1)],
            "kernels": kernels, "launches_per_step": plan.num_launches,
            "ramp": {"ms": round(ramp_s * 1e3, 1), "execs": n_ramp},
            "roofline": {
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "frac_source": "algorithmic bytes / ms_per_step of the timed steps",
                # the separate HIP-event loop (--full)
                "frac_hip_events": round(algo_bytes / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if full else None,
                "copy": copy,
                "traffic": traffic[0] if traffic else None,
                "traffic_source": (traffic[1] if traffic[1].startswith("live") else
                                   traffic[1] + " (committed rocprofv3 --pmc passes of this command)") if traffic else None,
                "kernel": "+".join(kernels), "algorithmic_bytes_per_launch": algo_bytes,
                "launch_ms_hip_events": round(launch_ms, 5) if full else None,
            },
        }

    def run_real_shape(self, shape, steps, warmup):
        """real input (C_in = 1) -> full complex spectrum, the mode the reference's bench.mojo times"""
        torch, mf = self.torch, self.mf
        gen = torch.Generator(device=self.dev).manual_seed(4321 + self.rank)
        x = torch.randn(tuple(shape) + (1,), generator=gen, device=self.dev, dtype=self.tdt)
        out = torch.empty(tuple(shape) + (2,), device=self.dev, dtype=self.tdt)
        plan = mf.plan_fft(self.tdt, self.tdt, x.shape, out.shape, ctx=self.ctx)
        elapsed, _, _ = self.timed(lambda: mf.fft(out, x, self.ctx, plan=plan), steps, warmup)
        launch_ms = mf.time_fft(out, x, plan=plan, iters=max(10, min(steps, 200)), ctx=self.ctx)
        elems = 1
        for d in shape:
            elems *= d
        algo_bytes = 3.0 * self.esz * elems  # one real read + one complex write per point
        return {"shape": list(shape) + [1], "ms_per_step": round(elapsed * 1e3 / steps, 5),
                "launch_ms_hip_events": round(launch_ms, 5),
                "kernels": [plan.kernel_name(d) for d in range(len(shape) - 1)],
                "algorithmic_bytes_per_launch": algo_bytes,
                "roofline_frac": round(algo_bytes / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    # ---- strong scaling: ONE config-5 batch over all ranks ----------------------------
    def strong_leg(self, steps, warmup, dump_dir=None):
        torch, mf = self.torch, self.mf
        from hackathon_fft_amd.dist import ShardedFFT, all_shard_bounds
        shape, bases, _ = WORKLOADS[STRONG_WORKLOAD]
        gshape = tuple(shape) + (2,)
        sharded = ShardedFFT(self.tdt, self.tdt, gshape, gshape, bases=bases, device=self.dev_index)
        counts = [c for _, c in all_shard_bounds(shape[0], self.world)]
        gen = torch.Generator(device=self.dev).manual_seed(4321 + self.rank)
        x_slab = torch.randn(sharded.slab_in_shape, generator=gen, device=self.dev, dtype=self.tdt)
        out_slab = torch.empty_like(x_slab)
        t_res, _, _ = self.timed(lambda: sharded.fft(out_slab, x_slab), steps, warmup)
        if dump_dir and self.rank == 0:
            dump_outputs(dump_dir, out_slab)
        ms_res = t_res * 1e3 / steps
        flops = flops_5nlogn(shape)
        leg = {
            "workload": STRONG_WORKLOAD, "baseline_config_index": 4, "scaling": "strong", "n_gpus": self.world,
            "volumes_per_rank": counts, "ideal_speedup_vs_1gpu": round(shape[0] / max(counts), 3),
            "compute_shards_resident": {"ms_per_step": round(ms_res, 5), "gflops": round(flops / (ms_res * 1e-3) / 1e9, 2),
                                        "steps": steps, "kernel_choice": "for the whole batch (bit-identical to 1 GPU)"},
            "compute_shards_resident_own_size": None, "end_to_end_from_root": None, "model": None,  # --full
            "kernels": [sharded._backend.plan.kernel_name(d) for d in range(len(shape) - 1)] if sharded.count else [],
        }
        if not self.args.full:
            return leg
        # end to end from a root-held tensor: scatter (grouped P2P over RCCL / xGMI), transform, gather
        x_full = out_full = None
        if self.rank == 0:
            x_full = torch.randn(gshape, generator=gen, device=self.dev, dtype=self.tdt)
            out_full = torch.empty_like(x_full)
        e2e_steps = max(3, min(steps, 20))
        for _ in range(2):
            sharded.fft_from_root(out_full, x_full, root=0, device=self.dev)
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(e2e_steps):
            sharded.fft_from_root(out_full, x_full, root=0, device=self.dev)
        self.barrier()
        t_e2e = self.allmax(time.perf_counter() - t0)
        ms_e2e = t_e2e * 1e3 / e2e_steps
        # the same resident-shard leg with every rank choosing its kernels for ITS OWN slab size (match_single_gpu=False:
        # results agree with the single-GPU plan to rounding, not bit for bit; the default pays 6-9 % on cache-resident
        # slabs for bit-identity, hackathon_fft_amd/dist.py)
        own = None
        if self.world > 1:
            sh2 = ShardedFFT(self.tdt, self.tdt, gshape, gshape, bases=bases, device=self.dev_index, match_single_gpu=False)
            t_own, _, _ = self.timed(lambda: sh2.fft(out_slab, x_slab), steps, warmup)
            own = {"ms_per_step": round(t_own * 1e3 / steps, 5), "gflops": round(flops / (t_own / steps) / 1e9, 2),
                   "kernels": [sh2._backend.plan.kernel_name(d) for d in range(len(shape) - 1)] if sh2.count else []}
        # what the end-to-end leg can reach at best: bytes per link / 153 GB/s each way, around the compute
        vol_bytes = 1.0
        for d in shape[1:]:
            vol_bytes *= d
        vol_bytes *= 2 * self.esz
        link_gbs = 153.0
        peer_counts = [c for r, c in enumerate(counts) if r != 0]
        t_link = (max(peer_counts) * vol_bytes / (link_gbs * 1e9) * 1e3) if peer_counts else 0.0   # ms, one direction
        t_comp = ms_res  # max-over-ranks compute of the resident shards, measured above
        model = None if not peer_counts else {
            "link_GBs_assumed": link_gbs, "bytes_per_volume": vol_bytes,
            "scatter_ms": round(t_link, 4), "gather_ms": round(t_link, 4), "compute_ms": round(t_comp, 4),
            "serial_ms": round(2 * t_link + t_comp, 4),
            # per-volume chunks, results returning on their own communicator: the first volume out, the last one back,
            # everything else overlapped on full-duplex links
            "pipelined_ms": round(t_link + (vol_bytes / (link_gbs * 1e9) * 1e3 if peer_counts else 0.0) +
                                  t_comp / max(1, max(counts)), 4),
            "ideal_compute_speedup": round(shape[0] / max(counts), 3),
            "note": "root-held 10 x 128^3: one volume is 16.8 MB = 0.11 ms per link and direction against ~0.011 ms of "
                    "compute, so end to end this leg is transfer-bound by construction; compute_shards_resident is the "
                    "strong-scaling figure of the transform itself",
        }
        leg.update({
            "compute_shards_resident_own_size": own,
            "end_to_end_from_root": {"ms_per_step": round(ms_e2e, 5), "gflops": round(flops / (ms_e2e * 1e-3) / 1e9, 2),
                                     "steps": e2e_steps,
                                     "transport": ("gloo, host-staged (rehearsal)" if self.rehearse else
                                                   "RCCL: per-volume chunks, grouped sends root -> peers, results on a "
                                                   "second communicator" if self.world > 1 else
                                                   "none (one rank owns the whole batch)")},
            "model": model,
        })
        return leg


def worker(args, json_out, live_traffic=None):
    b = Bench(args)
    b.live_traffic = live_traffic or {}
    mf = b.mf
    strong = args.scaling == "strong"
    name = args.workload or (STRONG_WORKLOAD if strong else DEFAULT_WORKLOAD)
    shape, bases, cfg_idx = WORKLOADS[name]
    result = {"metric": METRIC}
    if strong:
        leg = b.strong_leg(args.steps, args.warmup, dump_dir=args.dump_outputs)
        r = leg["compute_shards_resident"]
        result.update({
            "value": r["gflops"], "unit": "GFLOP/s", "n_gpus": b.world, "ranks_seen": b.ranks_seen,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": r["ms_per_step"],
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": STRONG_WORKLOAD, "baseline_config_index": 4,
                       "parallelism": f"one 10 x 128^3 batch split {leg['volumes_per_rank']} over {b.world} ranks",
                       "input": "complex64 N(0,1), resident in HBM"},
            "strong_config5": leg,
        })
    else:
        if b.distributed:
            # weak scaling: the global problem is world x (per-GPU shape); every rank owns one resident slab
            from hackathon_fft_amd.dist import ShardedFFT
            gshape = (shape[0] * b.world,) + tuple(shape[1:]) + (2,)
            sharded = ShardedFFT(b.tdt, b.tdt, gshape, gshape, bases=bases, device=b.dev_index)
            x, out = b.make_input(shape)
            assert sharded.slab_in_shape == tuple(x.shape)
            main = b.run_workload(name, args.steps, args.warmup, plan=sharded._backend.plan, x=x, out=out,
                                  dump_dir=args.dump_outputs)
        else:
            main = b.run_workload(name, args.steps, args.warmup, dump_dir=args.dump_outputs)
        n_gpus = b.world
        value = flops_5nlogn(shape) * n_gpus / (main["ms_per_step"] * 1e-3) / 1e9
        result.update({
            "value": round(value, 2), "unit": "GFLOP/s", "n_gpus": n_gpus, "ranks_seen": b.ranks_seen,
            "steps": args.steps, "warmup": args.warmup, "ramp": main["ramp"],
            "ms_per_step": main["ms_per_step"], "us_per_transform": round(main["ms_per_step"] * 1e3 / shape[0], 6),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {
                "workload": name, "baseline_config_index": cfg_idx, "shape_per_gpu": main["shape"],
                "bases": main["bases"], "stages": main["stages"], "kernels": main["kernels"],
                "launches_per_step": main["launches_per_step"],
                "parallelism": f"batch-sharded x{n_gpus}, no data-path collective" + (" (rehearsal: ranks share GPUs)" if b.rehearse else ""),
                "input": ("real fp N(0,1) (C_in = 1), full complex spectrum out" if name.endswith("_real") else
                          "complex64 N(0,1)") + ", seed 1234+rank, resident in HBM",
            },
            "roofline": main["roofline"],
        })
        del main
        b.torch.cuda.empty_cache()
        if (args.full and not args.no_strong_leg and name == DEFAULT_WORKLOAD and args.dtype == "f32" and
                not args.faithful):
            # The headline above is complete; the strong-scaling leg is an extra object and must never cost the line.
            # It is the only part of the run with point-to-point traffic between GPUs, so a watchdog bounds it: if it
            # has not finished in time, every rank leaves (rank 0 prints the line without the leg first).
            import threading

            def bail():
                if b.rank == 0:
                    result["strong_config5"] = {"error": "strong-scaling leg did not finish within 120 s; skipped"}
                    json_out.write(json.dumps(result) + "\n")
                    json_out.flush()
                os._exit(0)

            watchdog = threading.Timer(120.0, bail)
            watchdog.daemon = True
            watchdog.start()
            try:
                result["strong_config5"] = b.strong_leg(max(10, min(args.steps, 100)), max(2, min(args.warmup, 10)))
            except Exception as e:  # an RCCL / allocation error in the extra leg is reported, not fatal
                result["strong_config5"] = {"error": repr(e)[:300]}
            finally:
                watchdog.cancel()
        if (args.full and b.world == 1 and not args.no_configs and name == DEFAULT_WORKLOAD and args.dtype == "f32" and
                not args.faithful):
            cfgs = []
            for w in OTHER_BASELINE_CONFIGS:
                c = b.run_workload(w, args.steps, args.warmup)
                c.pop("shape", None)
                cfgs.append(c)
                b.torch.cuda.empty_cache()
            result["configs"] = sorted(cfgs, key=lambda c: c["baseline_config_index"])
            rf = []
            for shp in RFFT_REFERENCE_SHAPES:
                rf.append(b.run_real_shape(shp, max(10, min(args.steps, 100)), max(2, min(args.warmup, 10))))
                b.torch.cuda.empty_cache()
            result["rfft_reference_bench"] = rf
    if b.rank == 0:
        if args.full and b.world == 1 and not args.no_cpu_baseline and args.dtype == "f32":
            result["cpu_baseline"] = cpu_baseline(shape, bases)
        want_vendor = args.vendor if args.vendor is not None else (
            b.world == 1 and name == DEFAULT_WORKLOAD and not strong and args.dtype == "f32" and not args.faithful)
        if args.full and want_vendor and b.world == 1:
            b.torch.cuda.synchronize()
            result["vendor_rocfft"] = vendor_compare()
        json_out.write(json.dumps(result) + "\n")
        json_out.flush()
    if b.distributed:
        b.dist.barrier()
        b.dist.destroy_process_group()


def main():
    # the host driver of this pool only supports dmabuf IPC: without it RCCL fails in hipIpcGetMemHandle (set before HIP starts)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    json_out = _claim_stdout()
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args, json_out))  # nothing in this process has touched torch or the GPU
    live = {}
    headline = (args.workload or DEFAULT_WORKLOAD) == DEFAULT_WORKLOAD and args.scaling == "weak"
    # never from inside a profiler run: its preloaded tool library has initialised the GPU in THIS process already, and
    # the child rocprofv3 would exec python3 out of an initialised process (the GPU pool refuses that exec)
    under_profiler = ("rocprofiler" in os.environ.get("LD_PRELOAD", "") or
                      any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ))
    if (args.full and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and headline and
            not args.no_live_pmc and args.dtype == "f32" and not args.faithful and not under_profiler):
        # child processes under rocprofv3; this process has not touched the GPU yet.  Bounded: one failed or slow pass
        # ends the collection (the committed profiles are the fallback), and the whole of it gets at most 2 minutes
        t_live = time.perf_counter()
        for w in [DEFAULT_WORKLOAD] + ([] if args.no_configs else OTHER_BASELINE_CONFIGS):
            left = 120.0 - (time.perf_counter() - t_live)
            if left < 10.0:
                break
            t = live_pmc_traffic(w, timeout_s=min(60.0, left))
            if not t:
                break
            live[w] = t
    worker(args, json_out, live)


if __name__ == "__main__":
    main()
