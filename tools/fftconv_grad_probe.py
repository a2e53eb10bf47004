"""The fused filter gradient of fftconv (mf.plan_fftconv_grad; TileCfg::WGRAD, the MIFFT_CONV_GRAD_TAG payload) and the backward
of the differentiable mf.fftconv beside their yardsticks, in one process per run, at the shapes the README reports for fftconv:
  (a) the filter-gradient kernel (one launch, x and gy read once, channels * partials rows of bins written) plus the sum of
      its partials and the irfftn of the channels' rows -- plan.filter_grad -- against the composition it replaces, built from
      the library's own operations: pad both tensors to the FFT length, rfftn(onesided=True) twice, conj(U) * G, the sum over
      the batch, irfftn, the crop.  (a0) is the kernel's launch alone.  The long rows have no single FFT length the packed
      rows take: their composition is the same one on overlap-save blocks, which torch cuts (pad and unfold for the
      u-blocks; pad, reshape and pad for the g-blocks) before the two rfftn of (rows * blocks, n).
  (b) the whole backward of the gated op (x, k, pregate, postgate, skip all wanting gradients) through mf.fftconv's
      autograd.Function against the same backward composed from torch autograd over torch.fft (the forward graph built once,
      the backward timed).
  (c) what binds: two R2C row launches of the same padded rows (the library's rfftn), and a copy of the kernel's bytes.
Before any timing (a) is compared with its composition (the worst channel's relative l2).
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition printed per shape: the fused filter gradient's median is not above the composition's by more than the spread
(max - min) of the composition's own windows.
    python tools/fftconv_grad_probe.py [out.txt]        (default: profiles/r19_fftconv_grad.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L, K, n, overlap-save, dtype)
SHAPES = [(8, 768, 8192, 8192, 16384, False, torch.float32), (64, 256, 1024, 1024, 2048, False, torch.float32),
          (64, 256, 1024, 1024, 2048, False, torch.float64), (8 * 768, 1, 8192, 8192, 16384, False, torch.float32),
          (32, 1, 480000, 257, 4096, True, torch.float32), (32, 1, 480000, 4097, 16384, True, torch.float32)]
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_fftconv_grad.txt")
    lines = [f"# tools/fftconv_grad_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes of the kernel = x and gy read once each; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median (a) <= median (a composition) + (max - min of the composition's windows)"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<44} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    for B, D, L, K, n, ols, dtype in SHAPES:
        tname = "fp32" if dtype == torch.float32 else "fp64"
        esz = 4 if dtype == torch.float32 else 8
        say(f"{B}x{D}x{L} K={K} n={n} {'overlap-save' if ols else 'single block'} {tname}")
        rows = B * D
        x = torch.randn(B, D, L, device=DEV, dtype=dtype)
        gy = torch.randn(B, D, L, device=DEV, dtype=dtype)
        plan = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=K if ols else None)
        xr, gr = x.reshape(plan.in_shape), gy.reshape(plan.grad_shape)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        nc = n if not ols else 1 << (L + K - 2).bit_length()  # (the FFT length of (b)'s torch composition)
        Fb, S, c = (plan.blocks, plan.step, K - 1) if ols else (1, L, 0)
        pad = torch.nn.functional.pad

        def padded():
            """the rows the composition transforms: (rows * blocks, n) each"""
            if not ols:
                return pad(x, (0, n - L)).reshape(rows, n), pad(gy, (0, n - L)).reshape(rows, n)
            xb = pad(x, (c, (Fb - 1) * S + n - c - L)).unfold(-1, n, S)                    # block f: samples f S - c .. of the row
            gb = pad(pad(gy, (0, Fb * S - L)).reshape(B, D, Fb, S), (c, n - c - S))         # what block f stored, put back at c
            return xb.reshape(rows * Fb, n), gb.reshape(rows * Fb, n)

        def composed_gk():
            xp, gp = padded()
            U, G = mf.rfftn(xp, onesided=True), mf.rfftn(gp, onesided=True)
            A = (U.conj() * G).reshape(B, D, Fb, n // 2 + 1).sum(dim=(0, 2))
            return mf.irfftn(A, n)[:, :K]

        xp, gp = (t.contiguous() for t in padded())
        src = torch.empty(rows * L, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        variants = {"kernel": lambda: plan.run(out, xr, gr), "fused": lambda: plan.filter_grad(xr, gr, K),
                    "r2c2": lambda: (mf.rfftn(xp, onesided=True), mf.rfftn(gp, onesided=True)), "copy": lambda: dst.copy_(src)}
        try:
            ref = composed_gk().double()
            got = plan.filter_grad(xr, gr, K).double()
            err = float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max())
            variants["composition"] = composed_gk
        except mf.MifftError as e:
            err = None
            say(f"  the composition is not available at this shape: {e}")
        # (b) the whole backward, all five gradients
        a, b = (torch.randn(B, D, L, device=DEV, dtype=dtype).requires_grad_(True) for _ in range(2))
        k = (torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5).requires_grad_(True)
        d = torch.randn(D, device=DEV, dtype=dtype).requires_grad_(True)
        xs = x.clone().requires_grad_(True)
        ins = (xs, k, a, b, d)
        y_mf = mf.fftconv(xs, k, pregate=a, postgate=b, skip=d, **({"block": n} if ols else {"n": n}))
        y_th = b * torch.fft.irfft(torch.fft.rfft(a * xs, n=nc) * (torch.fft.rfft(k, n=nc) + d.reshape(D, 1)), n=nc)[..., :L]
        variants["backward"] = lambda: torch.autograd.grad(y_mf, ins, gy, retain_graph=True)
        variants["backward composed"] = lambda: torch.autograd.grad(y_th, ins, gy, retain_graph=True)
        t = measure(variants)
        nbytes = 2 * rows * L * esz
        geo = plan.pass_geometry(1)
        row("(a0) the kernel's launch alone", t["kernel"],
            f"{nbytes / 1e6:.1f} MB  {nbytes / (t['kernel'][0] * 1e-3) / PEAK * 100:.1f} % of 8 TB/s  {plan.kernel_name(1)} "
            f"partials={plan.partials} geometry={geo}" + (f" blocks per row {plan.blocks} step {plan.step}" if ols else ""))
        row("(a) fused filter gradient (+ sum, irfftn)", t["fused"])
        if "composition" in t:
            row("(a) composition: pad, 2 rfftn, conj *, sum, irfftn", t["composition"], f"on ({rows * Fb}, {n}); worst channel rel l2 of (a) against it {err:.2e}")
        row("(b) backward of the gated op, five gradients", t["backward"])
        row("(b) the same backward by torch autograd on torch.fft", t["backward composed"], f"at n = {nc}")
        row("(c) two R2C row launches of the padded rows", t["r2c2"], f"rfftn of ({rows * Fb}, {n}) twice")
        row("(c) copy of the kernel's bytes", t["copy"], "torch copy_ of x's elements: read + written = x + gy")
        say(f"  ratios: (a0) / two R2C {ratio(t['kernel'], t['r2c2'])}   (a0) / copy {ratio(t['kernel'], t['copy'])}   "
            f"(b) / (b composed) {ratio(t['backward'], t['backward composed'])}")
        if "composition" in t:
            ta, tb = t["fused"], t["composition"]
            met = ta[0] <= tb[0] + (tb[2] - tb[1])
            say(f"  ratio (a) / (a composition) {ratio(ta, tb)}")
            say(f"  condition: {ta[0]:.4f} <= {tb[0]:.4f} + {tb[2] - tb[1]:.4f}: {'met' if met else 'MISSED'}")
        del x, gy, xr, gr, out, xp, gp, src, dst, a, b, k, d, xs, ins, y_mf, y_th, variants, plan
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
