"""The convolution of two signal batches (mf.plan_fftconv_pair / mf.fftconv_pair; TileCfg::PAIR, the MIFFT_CONV_PAIR_TAG payload)
beside its yardsticks, in one process per run, mode "full" (Lo = L + K - 1):
  (a) the composition it replaces inside this library: pad v to the FFT length, rfftn(onesided=True) -- one launch, a
      (rows, n / 2 + 1) spectrum in memory -- then a plan_fftconv with D = rows, set_filter_spectrum and its launch.
  (b) torch.fft.rfft of both, the product, torch.fft.irfft, the crop.
  (c) what binds: an R2C row launch plus a C2R row launch of the same rows (the library's rfftn and irfftn).
  (d) a copy of the kernel's bytes (x and v read, out written).
  and the backward of mf.fftconv_pair (both gradients) against torch autograd over (b), the forward graphs built once.
Before any timing the kernel is compared with (b) in float64 (the worst row's relative l2).
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition printed per shape: the kernel's median is not above (a)'s by more than the spread (max - min) of (a)'s own windows.
    python tools/fftconv_pair_probe.py [out.txt]        (default: profiles/r28_fftconv_pair.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (rows, L, K, n, dtype, x is v)
SHAPES = [(6144, 8192, 8192, 16384, torch.float32, False), (16384, 1024, 1024, 2048, torch.float32, False),
          (16384, 1024, 1024, 2048, torch.float64, False), (32, 8192, 257, 16384, torch.float32, False),
          (16384, 1024, 1024, 2048, torch.float32, True)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, WARM = 7, 10, 2
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


def ratio(a, b):
    """median a / median b with the spread the run shows: [min a / max b .. max a / min b]"""
    return f"{a[0] / b[0]:.3f} [{a[1] / b[2]:.3f} .. {a[2] / b[1]:.3f}]"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r28_fftconv_pair.txt")
    lines = [f"# tools/fftconv_pair_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes of the kernel = x and v read once each, out written once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median (kernel) <= median (a) + (max - min of (a)'s windows)"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<52} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    for rows, L, K, n, dtype, same in SHAPES:
        tname = "fp32" if dtype == torch.float32 else "fp64"
        esz = 4 if dtype == torch.float32 else 8
        Lo = L + K - 1
        say(f"{rows}x{L} against {rows}x{K} n={n} Lo={Lo} {tname}" + (" (x is v)" if same else ""))
        x = torch.randn(rows, L, device=DEV, dtype=dtype)
        v = x if same else torch.randn(rows, K, device=DEV, dtype=dtype)
        plan = mf.plan_fftconv_pair(dtype, rows, L, K, n, out_length=Lo)
        xr, vr = x.reshape(plan.in_shape), v.reshape(plan.v_shape)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        cplan = mf.plan_fftconv(dtype, 1, rows, L, n, out_length=Lo)  # (D = rows: every row its own filter row)
        cout = torch.empty(cplan.out_shape, device=DEV, dtype=dtype)
        pad = torch.nn.functional.pad

        def composed():
            cplan.set_filter_spectrum(mf.rfftn(pad(v, (0, n - K)), onesided=True))
            mf.fft(cout, xr, plan=cplan)
            return cout

        def by_torch(a=x, b=v):
            return torch.fft.irfft(torch.fft.rfft(a, n=n) * torch.fft.rfft(b, n=n), n=n)[..., :Lo]

        xp = pad(x, (0, n - L)).contiguous()
        spec = mf.rfftn(xp, onesided=True)
        nbytes = rows * (L + (0 if same else K) + Lo) * esz
        src = torch.empty(nbytes // esz // 2, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        plan.run(out, xr, vr)
        ref = by_torch(x.double(), v.double())
        err = float(((out[..., 0].double() - ref).norm(dim=1) / ref.norm(dim=1)).max())
        erra = float(((composed()[..., 0].double() - ref).norm(dim=1) / ref.norm(dim=1)).max())
        del ref
        variants = {"kernel": lambda: plan.run(out, xr, vr), "a": composed, "b": by_torch,
                    "c": lambda: (mf.rfftn(xp, onesided=True), mf.irfftn(spec, n)), "copy": lambda: dst.copy_(src)}
        # the backward: both gradients
        gy = torch.randn(rows, Lo, device=DEV, dtype=dtype)
        xs = x.clone().requires_grad_(True)
        vs = xs if same else v.clone().requires_grad_(True)
        ins = (xs,) if same else (xs, vs)
        y_mf = mf.fftconv_pair(xs, vs, n=n, mode="full")
        y_th = by_torch(xs, vs)
        variants["backward"] = lambda: torch.autograd.grad(y_mf, ins, gy, retain_graph=True)
        variants["backward torch"] = lambda: torch.autograd.grad(y_th, ins, gy, retain_graph=True)
        t = measure(variants)
        row("the kernel: one launch", t["kernel"],
            f"{nbytes / 1e6:.1f} MB  {nbytes / (t['kernel'][0] * 1e-3) / PEAK * 100:.1f} % of 8 TB/s  {plan.kernel_name(1)} "
            f"geometry={plan.pass_geometry(1)}  worst row rel l2 against (b) in fp64 {err:.2e}")
        row("(a) pad v, rfftn, set_filter_spectrum, plan_fftconv", t["a"], f"D = {rows}; its own rel l2 {erra:.2e}")
        row("(b) torch.fft.rfft x 2, product, irfft, crop", t["b"])
        row("(c) an R2C plus a C2R row launch of the same rows", t["c"], f"rfftn of ({rows}, {n}), irfftn of ({rows}, {n // 2 + 1})")
        row("(d) copy of the kernel's bytes", t["copy"], "torch copy_: read + written = x + v + out")
        row("backward of fftconv_pair, both gradients", t["backward"])
        row("the same backward by torch autograd over (b)", t["backward torch"])
        say(f"  ratios: kernel / (a) {ratio(t['kernel'], t['a'])}   kernel / (b) {ratio(t['kernel'], t['b'])}   "
            f"kernel / (c) {ratio(t['kernel'], t['c'])}   kernel / (d) {ratio(t['kernel'], t['copy'])}   "
            f"backward / torch {ratio(t['backward'], t['backward torch'])}")
        tk, ta = t["kernel"], t["a"]
        met = tk[0] <= ta[0] + (ta[2] - ta[1])
        say(f"  condition: {tk[0]:.4f} <= {ta[0]:.4f} + {ta[2] - ta[1]:.4f}: {'met' if met else 'MISSED'}")
        del x, v, xr, vr, out, cout, xp, spec, src, dst, gy, xs, vs, ins, y_mf, y_th, variants, plan, cplan
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
