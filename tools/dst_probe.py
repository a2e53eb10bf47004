"""DST rows (MIFFT_DST_TAG, MIFFT_DST_TYPE4_TAG) and the N-D DST beside their yardsticks, in one process per run:
  (a) dst rows against dct rows of the same type and shape: equal bytes and equal passes, so dct is the yardstick;
  (b) dst rows against the composition they replace: a torch sign multiply + mf.dct + flip;
  (c) dstn against dctn on 100x640x480 and 10x128^3.
The condition checked for (a) and (c): the sine plan is not slower than its cosine yardstick beyond the spread of the
yardstick's own repeated timings in this run -- median(dst) <= max over the yardstick's windows.  The yardstick is timed twice
in every round of the alternation ("dct" and "dct again"), which shows what two timings of the same plan differ by.
Timing: HIP events around windows of 20 calls, the variants of a shape alternating window by window inside the process, 5
warm-up calls each first; the figure is the median of 7 windows, the spread their min .. max.  Bytes are the kernels' own traffic
(rows: x once + out once; N-D: the same per transformed dim); the rate is given as a fraction of 8 TB/s.
    python tools/dst_probe.py [out.txt]        (default: profiles/r15_dst.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

ROW_SHAPES = [((100000, 1024), torch.float32, 2), ((500000, 128), torch.float32, 2), ((100000, 1024), torch.float64, 2),
              ((100000, 1024), torch.float32, 4)]
ND_SHAPES = [(100, 640, 480), (10, 128, 128, 128)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, WARM = 7, 20, 5
DEV = "cuda:0"


def measure(variants):
    """{name: fn} -> {name: (median ms, min ms, max ms)}: windows of CALLS calls, the variants alternating"""
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / CALLS)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def report(lines, label, t, nbytes, note):
    med, lo, hi = t
    frac = nbytes / (med * 1e-3) / PEAK
    lines.append(f"  {label:<26} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {note}")
    print(lines[-1], flush=True)


def ratio(a, b):
    """median a / median b with the spread the run shows: [min a / max b .. max a / min b]"""
    return f"{a[0] / b[0]:.3f} [{a[1] / b[2]:.3f} .. {a[2] / b[1]:.3f}]"


def verdict(lines, what, sine, cos, again):
    """the condition: median of the sine plan <= the slowest window of its yardstick (both timings of it)"""
    worst = max(cos[2], again[2])
    ok = sine[0] <= worst
    lines.append(f"  condition ({what} median {sine[0]:.4f} ms <= slowest yardstick window {worst:.4f} ms): "
                 f"{'holds' if ok else 'EXCEEDED'}")
    print(lines[-1], flush=True)


def probe_rows(lines):
    for shape, dtype, t in ROW_SHAPES:
        batch, n = shape
        esz = 4 if dtype == torch.float32 else 8
        lines.append(f"(a, b) type {t}, {batch}x{n} {'fp32' if dtype == torch.float32 else 'fp64'}:")
        print(lines[-1], flush=True)
        x = torch.randn(shape + (1,), device=DEV, dtype=dtype)
        out = torch.empty_like(x)
        nbytes = 2 * batch * n * esz
        ps = mf.plan_fft(dtype, dtype, x.shape, out.shape, dct=True, dst=True, dct_type=t)
        pc = mf.plan_fft(dtype, dtype, x.shape, out.shape, dct=True, dct_type=t)
        x2 = x.squeeze(-1)
        sign = (1 - 2 * (torch.arange(n, device=DEV) % 2)).to(dtype)

        def composed():
            return mf.dct(x2 * sign, type=t).flip(-1)

        ref = mf.dst(x2[:64], type=t)
        err = ((mf.dct(x2[:64] * sign, type=t).flip(-1) - ref).norm() / ref.norm()).item()
        ctx = mf.DeviceContext(0)
        tm = measure({"dst": lambda: mf.fft(out, x, ctx, plan=ps), "dct": lambda: mf.fft(out, x, ctx, plan=pc),
                      "composition": composed, "again": lambda: mf.fft(out, x, ctx, plan=pc)})
        report(lines, f"dst(type={t})", tm["dst"], nbytes, ps.kernel_name(0))
        report(lines, f"dct(type={t})", tm["dct"], nbytes, pc.kernel_name(0))
        report(lines, f"dct(type={t}) again", tm["again"], nbytes, "the same plan, timed a second time in every round")
        report(lines, "composition", tm["composition"], nbytes, f"x * sign + mf.dct + flip (agrees with dst to {err:.1e})")
        lines.append(f"  ratios: dst / dct {ratio(tm['dst'], tm['dct'])}   dct again / dct {ratio(tm['again'], tm['dct'])}   "
                     f"composition / dst {ratio(tm['composition'], tm['dst'])}")
        print(lines[-1], flush=True)
        verdict(lines, "dst", tm["dst"], tm["dct"], tm["again"])
        del x, out, x2, ps, pc
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def probe_nd(lines):
    dtype = torch.float32
    for shape in ND_SHAPES:
        lines.append(f"(c) {'x'.join(str(v) for v in shape)} fp32, every dim but the first:")
        print(lines[-1], flush=True)
        x = torch.randn(shape + (1,), device=DEV, dtype=dtype)
        out = torch.empty_like(x)
        nbytes = 2 * x.numel() * 4 * (len(shape) - 1)
        ps = mf.plan_fft(dtype, dtype, x.shape, out.shape, dctn=True, dst=True)
        pc = mf.plan_fft(dtype, dtype, x.shape, out.shape, dctn=True)
        ctx = mf.DeviceContext(0)
        tm = measure({"dstn": lambda: mf.fft(out, x, ctx, plan=ps), "dctn": lambda: mf.fft(out, x, ctx, plan=pc),
                      "again": lambda: mf.fft(out, x, ctx, plan=pc)})
        report(lines, "dstn", tm["dstn"], nbytes, " ".join(ps.kernel_name(d) for d in range(ps.ndim)))
        report(lines, "dctn", tm["dctn"], nbytes, " ".join(pc.kernel_name(d) for d in range(pc.ndim)))
        report(lines, "dctn again", tm["again"], nbytes, "the same plan, timed a second time in every round")
        lines.append(f"  ratios: dstn / dctn {ratio(tm['dstn'], tm['dctn'])}   dctn again / dctn {ratio(tm['again'], tm['dctn'])}")
        print(lines[-1], flush=True)
        verdict(lines, "dstn", tm["dstn"], tm["dctn"], tm["again"])
        del x, out, ps, pc
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_dst.txt")
    lines = [f"# tools/dst_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = x + out of each launch, each moved once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio a / b = median a / median b [min a / max b .. max a / min b]"]
    probe_rows(lines)
    probe_nd(lines)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
