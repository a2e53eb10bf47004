"""The fused inverse MDCT (MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan) beside its yardsticks, in one process per run:
  (a) plan_imdct: one launch;
  (b) the composition it replaced (mf.api._imdct_composed): one DCT-IV launch + index_select + window + zeros + two shifted adds
      + slice;
  (c) the floor: the DCT-IV rows of the same frames alone (no unfold, no window, no overlap-add; it writes F * n values);
  (d) a copy of (a)'s bytes (torch copy_ of half as many elements as x and out together: read + written = (a)'s traffic).
Timing: HIP events around windows of 20 calls, the variants of a shape alternating window by window inside the process, 5
warm-up calls each first; the figure is the median of 7 windows, the spread their min .. max.  Bytes are the fused kernel's own
traffic (x once + out once); the rate is given as a fraction of 8 TB/s.
    python tools/imdct_probe.py [out.txt]        (default: profiles/r14_imdct.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

SHAPES = [((32, 480000), 256), ((32, 480000), 1024), ((2, 480000), 256)]
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


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_imdct.txt")
    lines = [f"# tools/imdct_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = x + out of the fused kernel, each moved once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio a / b = median a / median b [min a / max b .. max a / min b]"]
    dtype = torch.float32
    for (batch, T), n in SHAPES:
        lines.append(f"{batch}x{T} n={n} fp32:")
        print(lines[-1], flush=True)
        frames = mf.mdct_frames(T, n)
        X = torch.randn(batch, frames, n, 1, device=DEV, dtype=dtype)
        plan = mf.plan_imdct(dtype, batch, frames, n, length=T)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        nbytes = (batch * frames * n + batch * T) * 4
        w = mf.mdct_window(n)
        X3 = X.squeeze(-1)
        rows = X.reshape(batch * frames, n, 1)
        pf = mf.plan_fft(dtype, dtype, rows.shape, rows.shape, dct=True, dct_type=4)
        ro = torch.empty_like(rows)
        src = torch.empty((batch * frames * n + batch * T) // 2, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        ctx = mf.DeviceContext(0)
        mf.fft(out, X, ctx, plan=plan)
        ref = mf.api._imdct_composed(X3, w, False, T)
        err = ((ref - out.squeeze(-1)).norm() / ref.norm()).item()
        del ref
        t = measure({"imdct": lambda: mf.fft(out, X, ctx, plan=plan),
                     "composition": lambda: mf.api._imdct_composed(X3, w, False, T),
                     "floor": lambda: mf.fft(ro, rows, ctx, plan=pf),
                     "copy": lambda: dst.copy_(src)})
        sched = mf.istft_schedule(plan)
        note = (f"{plan.kernel_name(2)} geometry={plan.pass_geometry(2)} runs of {min(r[1] for r in sched)}..{max(r[1] for r in sched)} "
                f"tiles, {sum(r[2] for r in sched)} warm-up frames")
        report(lines, "(a) plan_imdct", t["imdct"], nbytes, note)
        report(lines, "(b) composition", t["composition"], nbytes,
               f"dct(type=4) + index_select + window + zeros + 2 adds + slice (agrees with (a) to {err:.1e})")
        report(lines, "(c) floor: dct4 rows", t["floor"], 2 * batch * frames * n * 4, pf.kernel_name(0))
        report(lines, "(d) copy of (a)'s bytes", t["copy"], nbytes, "torch copy_ of nbytes / 2: read + written = nbytes")
        lines.append(f"  ratios: (a) / (b) {ratio(t['imdct'], t['composition'])}   (a) / (c) {ratio(t['imdct'], t['floor'])}   "
                     f"(a) / (d) {ratio(t['imdct'], t['copy'])}")
        print(lines[-1], flush=True)
        del X, out, rows, ro, src, dst, plan, pf
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
