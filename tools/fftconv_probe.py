"""The fused FFT convolution (mf.plan_fftconv; MIFFT_CONV_TAG) beside its yardsticks, in one process per run:
  (a) plan_fftconv: one launch, causal (offset 0, out_length L);
  (b) the composition it replaces: a zero-padded copy, mf.rfftn(onesided=True), a torch multiply by the filter spectrum,
      mf.irfftn, the crop to L samples (a contiguous copy).  The filter spectrum is precomputed for both sides;
  (c) the R2C rows and the C2R rows of the same n alone, one after the other (no padding, product or crop; they read and write
      whole rows of n reals and n / 2 + 1 bins);
  (d) a copy of (a)'s bytes (torch copy_ of half as many elements as x and y together: read + written = (a)'s traffic).
Every shape is B x D x L at the FFT length n; the first shape runs a second time with D = 1 (one filter row for every row of
the launch), which shows what the per-channel filter rows cost.
Timing: HIP events around windows of 20 calls, the variants of a shape alternating window by window inside the process, 5
warm-up calls each first; the figure is the median of 7 windows, the spread their min .. max.  Bytes are the fused kernel's own
traffic (x once + y once; the filter spectra come on top, D (n / 2 + 1) complex values); the rate is a fraction of 8 TB/s.
The condition printed per shape: the fused median is below the composition's median by more than the spread (max - min) of
the composition's own windows.
    python tools/fftconv_probe.py [out.txt]        (default: profiles/r16_fftconv.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L, n, dtype)
SHAPES = [(8, 768, 8192, 16384, torch.float32), (64, 256, 1024, 2048, torch.float32), (64, 256, 1024, 2048, torch.float64),
          (8 * 768, 1, 8192, 16384, torch.float32)]
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_fftconv.txt")
    lines = [f"# tools/fftconv_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = x + y of the fused kernel, each moved once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio a / b = median a / median b [min a / max b .. max a / min b]",
             "# condition: median (a) < median (b) - (max (b) - min (b))"]
    fused = {}
    for B, D, L, n, dtype in SHAPES:
        tname = "fp32" if dtype == torch.float32 else "fp64"
        esz = 4 if dtype == torch.float32 else 8
        lines.append(f"{B}x{D}x{L} n={n} {tname}:")
        print(lines[-1], flush=True)
        rows, K = B * D, L
        x = torch.randn(B, D, L, device=DEV, dtype=dtype)
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        plan = mf.plan_fftconv(dtype, B, D, L, n)
        plan.set_filter(k)
        xr = x.reshape(rows, L, 1)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        H = torch.view_as_complex(plan.filter_spectrum.clone())  # (D, n / 2 + 1): precomputed for both sides
        nbytes = 2 * rows * L * esz
        hbytes = D * (n // 2 + 1) * 2 * esz

        def composition():
            xp = torch.zeros(B, D, n, device=DEV, dtype=dtype)
            xp[..., :L] = x
            X = mf.rfftn(xp.reshape(rows, n), onesided=True).reshape(B, D, n // 2 + 1)
            Y = X * H
            return mf.irfftn(Y.reshape(rows, n // 2 + 1), n)[:, :L].contiguous()

        pr = mf.plan_fft(dtype, dtype, (rows, n, 1), (rows, n // 2 + 1, 2), half_spectrum=True)
        pc = mf.plan_fft(dtype, dtype, (rows, n // 2 + 1, 2), (rows, n, 1), inverse=True, half_spectrum=True)
        full = torch.randn(rows, n, 1, device=DEV, dtype=dtype)
        spec = torch.empty(rows, n // 2 + 1, 2, device=DEV, dtype=dtype)
        back = torch.empty(rows, n, 1, device=DEV, dtype=dtype)
        src = torch.empty(rows * L, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        ctx = mf.DeviceContext(0)

        def floor():
            mf.fft(spec, full, ctx, plan=pr)
            mf.fft(back, spec, ctx, plan=pc)

        mf.fft(out, xr, ctx, plan=plan)
        ref = composition()
        err = ((ref - out.reshape(rows, L)).norm() / ref.norm()).item()
        del ref
        t = measure({"fused": lambda: mf.fft(out, xr, ctx, plan=plan), "composition": composition, "floor": floor,
                     "copy": lambda: dst.copy_(src)})
        fused[(B * D, L, n, tname, D)] = t["fused"]
        report(lines, "(a) plan_fftconv", t["fused"], nbytes,
               f"{plan.kernel_name(1)} geometry={plan.pass_geometry(1)} filter spectra {hbytes / 1e6:.1f} MB")
        report(lines, "(b) composition", t["composition"], nbytes,
               f"pad + rfftn(onesided) + multiply + irfftn + crop (agrees with (a) to {err:.1e})")
        report(lines, "(c) r2c rows + c2r rows", t["floor"], 2 * (rows * n * esz + rows * (n // 2 + 1) * 2 * esz),
               f"{pr.kernel_name(0)} + {pc.kernel_name(0)} (their own bytes)")
        report(lines, "(d) copy of (a)'s bytes", t["copy"], nbytes, "torch copy_ of nbytes / 2: read + written = nbytes")
        a, b = t["fused"], t["composition"]
        met = a[0] < b[0] - (b[2] - b[1])
        lines.append(f"  ratios: (a) / (b) {ratio(a, b)}   (a) / (c) {ratio(a, t['floor'])}   (a) / (d) {ratio(a, t['copy'])}")
        print(lines[-1], flush=True)
        lines.append(f"  condition: {a[0]:.4f} < {b[0]:.4f} - {b[2] - b[1]:.4f}: {'met' if met else 'MISSED'}")
        print(lines[-1], flush=True)
        del x, k, out, H, full, spec, back, src, dst, plan, pr, pc
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    # the per-channel filter rows against one filter row for every row: the same rows, L and n
    for key, t in fused.items():
        one = fused.get(key[:4] + (1,))
        if key[4] != 1 and one is not None:
            lines.append(f"D = {key[4]} against D = 1 at {key[0]} rows x {key[1]}, n = {key[2]} {key[3]}: (a) / (a, D = 1) {ratio(t, one)}")
            print(lines[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
