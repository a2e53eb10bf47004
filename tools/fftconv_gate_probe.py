"""Gated fftconv (mf.plan_fftconv(pregate=True, postgate=True); the 16-word MIFFT_CONV_TAG payload) beside its yardsticks, in one
process per run, at the shapes the README reports for fftconv:
  (a) the gated plan with both gates, y = b * conv(a * x), one launch (a1 / a2: the plans with the pregate or the postgate alone);
  (b) the composition it replaces: x * a in torch, the ungated plan of the same shape, y * b in torch -- two elementwise
      launches, an intermediate of x's size and one of y's, allocated by torch's caching allocator as a caller's would be;
  (c) the ungated plan alone: (a) / (c) is what the gates cost;
  (d) a copy of (a)'s bytes (torch copy_ of as many elements as x and a together: read + written = x + a + y + b).
Every shape is B x D x L (causal: L samples out) with D filters; the single-block shapes run at the FFT length n, the long rows
as overlap-save blocks of n points (taps = K).  Before any timing (a) is compared with (b) bit for bit.
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.  Bytes are each variant's own
compulsory traffic -- (a): x, a, y and b once each; (c): x and y --; the rate is a fraction of 8 TB/s.
The condition printed per shape: the gated median is below the composition's by more than the spread (max - min) of the
composition's own windows.
    python tools/fftconv_gate_probe.py [out.txt]        (default: profiles/r18_fftconv_gate.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L, K, n, overlap-save, dtype)
SHAPES = [(8, 768, 8192, 8192, 16384, False, torch.float32), (64, 256, 1024, 1024, 2048, False, torch.float32),
          (64, 256, 1024, 1024, 2048, False, torch.float64), (32, 1, 480000, 257, 4096, True, torch.float32),
          (32, 1, 480000, 4097, 16384, True, torch.float32)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, WARM = 7, 20, 3
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
    lines.append(f"  {label:<30} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {note}")
    print(lines[-1], flush=True)


def ratio(a, b):
    """median a / median b with the spread the run shows: [min a / max b .. max a / min b]"""
    return f"{a[0] / b[0]:.3f} [{a[1] / b[2]:.3f} .. {a[2] / b[1]:.3f}]"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_fftconv_gate.txt")
    lines = [f"# tools/fftconv_gate_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = each variant's own compulsory traffic, every tensor moved once: (a) x + a + y + b, (a1) x + a + y, (a2) x + y + b,",
             "#         (b) as (a), (c) x + y; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median (a) < median (b) - (max (b) - min (b))"]
    ctx = mf.DeviceContext(0)
    for B, D, L, K, n, ols, dtype in SHAPES:
        tname = "fp32" if dtype == torch.float32 else "fp64"
        esz = 4 if dtype == torch.float32 else 8
        lines.append(f"{B}x{D}x{L} K={K} n={n} {'overlap-save' if ols else 'single block'} {tname}")
        print(lines[-1], flush=True)
        rows = B * D
        x = torch.randn(rows, L, 1, device=DEV, dtype=dtype)
        a = torch.randn(rows, L, 1, device=DEV, dtype=dtype)
        b = torch.randn(rows, L, 1, device=DEV, dtype=dtype)
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        one = rows * L * esz  # (bytes of one tensor: out_length = L)
        plans = {g: mf.plan_fftconv(dtype, B, D, L, n, taps=K if ols else None, pregate=bool(g & 1), postgate=bool(g & 2))
                 for g in (0, 1, 2, 3)}
        for p in plans.values():
            p.set_filter(k)
        outs = {g: torch.empty(plans[g].out_shape, device=DEV, dtype=dtype) for g in plans}
        yb = torch.empty(plans[0].out_shape, device=DEV, dtype=dtype)

        def composition():
            mf.fft(yb, x * a, ctx, plan=plans[0])
            return yb * b

        src = torch.empty(2 * rows * L, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        variants = {"gated": lambda: plans[3].run(outs[3], x, pregate=a, postgate=b),
                    "pregate": lambda: plans[1].run(outs[1], x, pregate=a),
                    "postgate": lambda: plans[2].run(outs[2], x, postgate=b),
                    "composition": composition,
                    "ungated": lambda: mf.fft(outs[0], x, ctx, plan=plans[0]),
                    "copy": lambda: dst.copy_(src)}
        # agreement before any timing: bit for bit
        variants["gated"]()
        same = bool(torch.equal(outs[3], composition()))
        t = measure(variants)
        geo = f"geometry={plans[3].pass_geometry(1)}" + (f" blocks per row {plans[3].blocks} step {plans[3].step}" if ols else "")
        report(lines, "(a) gated, both gates", t["gated"], 4 * one, f"{plans[3].kernel_name(1)} {geo}")
        report(lines, "(a1) pregate alone", t["pregate"], 3 * one, plans[1].kernel_name(1))
        report(lines, "(a2) postgate alone", t["postgate"], 3 * one, plans[2].kernel_name(1))
        report(lines, "(b) composition", t["composition"], 4 * one,
               f"x * a + {plans[0].kernel_name(1)} + y * b ((a) equals it bit for bit: {same})")
        report(lines, "(c) ungated alone", t["ungated"], 2 * one, plans[0].kernel_name(1))
        report(lines, "(d) copy of (a)'s bytes", t["copy"], 4 * one, "torch copy_ of x's and a's elements: read + written = (a)'s bytes")
        ta, tb, tc = t["gated"], t["composition"], t["ungated"]
        met = ta[0] < tb[0] - (tb[2] - tb[1])
        lines.append(f"  ratios: (a) / (b) {ratio(ta, tb)}   (a) / (c) {ratio(ta, tc)}   (a1) / (c) {ratio(t['pregate'], tc)}   "
                     f"(a2) / (c) {ratio(t['postgate'], tc)}   (a) / (d) {ratio(ta, t['copy'])}   (c) / copy of (c)'s bytes "
                     f"{tc[0] / (t['copy'][0] / 2):.3f}")
        print(lines[-1], flush=True)
        lines.append(f"  the gates cost (a) - (c) = {ta[0] - tc[0]:.4f} ms; a copy of their bytes (two tensors read) takes about "
                     f"{t['copy'][0] / 2:.4f} ms; the elementwise passes of (b) cost (b) - (c) = {tb[0] - tc[0]:.4f} ms")
        print(lines[-1], flush=True)
        lines.append(f"  condition: {ta[0]:.4f} < {tb[0]:.4f} - {tb[2] - tb[1]:.4f}: {'met' if met else 'MISSED'}")
        print(lines[-1], flush=True)
        del x, a, b, k, plans, outs, yb, src, dst, variants
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
