"""Overlap-save fftconv (mf.plan_fftconv(taps=); the 12-word MIFFT_CONV_TAG payload) beside its yardsticks, in one process per run:
  (a) the fused plan, causal (offset 0, out_length T), at the block length fftconv_block(K) picks and at the power of two on
      either side of it (where one exists: K <= n - 1, n <= 16384, float64 8192);
  (b) the composition it replaces, built from this library at the picked block length n, S = n - K + 1: a zero-padded copy,
      unfold(-1, n, S) made contiguous (blocks of a batch entry side by side, so that a launch row's filter is row % D), the
      single-block plan_fftconv(offset=K - 1, out_length=S) over all blocks, and the reshape and crop to T samples (a
      contiguous copy).  The filter spectrum is precomputed for both sides;
  (c) torch.fft.rfft / irfft at the full length (scipy.fft.next_fast_len(T + K - 1)), product and crop included, the filter
      spectrum precomputed;
  (d) a copy of (a)'s bytes (torch copy_ of half as many elements as x and y together: read + written = (a)'s traffic).
Every shape is B x D x T with D filters of K taps.
A sweep follows: 32 x 480000 with a filter of 33 taps at every power of two from 256 to 16384 (float64: 8192), fused plans
only.  With so short a filter nearly every block sample is stored, so time * S / n, the time per block sample, is the cost of a
block of n points itself: the weights w(n) of fftconv_block's rule are these, relative to the cheapest.
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.  Bytes are the fused kernel's
own compulsory traffic (x once + y once); the rate is a fraction of 8 TB/s.
The condition printed per shape: the fused median at the picked block is not above the composition's median by more than the
spread (max - min) of the composition's own windows.
    python tools/fftconv_long_probe.py [out.txt]        (default: profiles/r17_fftconv_long.txt)"""
import os
import statistics
import sys

import scipy.fft
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, T, K, dtype)
SHAPES = [(32, 1, 480000, 257, torch.float32), (32, 1, 480000, 4097, torch.float32), (8, 768, 65536, 1025, torch.float32),
          (32, 1, 480000, 1025, torch.float64)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, WARM = 7, 10, 3
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


def candidates(K, dtype):
    """the block fftconv_block picks and the powers of two on either side of it that can hold the filter"""
    top = 8192 if dtype == torch.float64 else 16384
    n = mf.fftconv_block(K, dtype)
    return n, [m for m in (n // 2, n, 2 * n) if K <= m - 1 and m <= top]


def blocks_of(x, n, K):
    """(B, D, T) -> (B, F, D, n): the overlap-save blocks of every row, K - 1 zeros in front, zeros behind; one copy"""
    T = x.shape[-1]
    S = n - K + 1
    F = -(-T // S)
    xp = torch.nn.functional.pad(x, (K - 1, (F - 1) * S + n - (K - 1) - T))
    return xp.unfold(-1, n, S).permute(0, 2, 1, 3).contiguous()


def rows_of(y, T):
    """(B, F, D, S) -> (B, D, T): the blocks' stored parts side by side, cropped; one copy"""
    B, F, D, S = y.shape
    return y.permute(0, 2, 1, 3).reshape(B, D, F * S)[..., :T].contiguous()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_fftconv_long.txt")
    lines = [f"# tools/fftconv_long_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = x + y of the fused kernel, each moved once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio a / b = median a / median b [min a / max b .. max a / min b]",
             "# condition: median (a, picked block) <= median (b) + (max (b) - min (b))"]
    ctx = mf.DeviceContext(0)
    for B, D, T, K, dtype in SHAPES:
        tname = "fp32" if dtype == torch.float32 else "fp64"
        esz = 4 if dtype == torch.float32 else 8
        pick, cands = candidates(K, dtype)
        lines.append(f"{B}x{D}x{T} K={K} {tname}: fftconv_block picks {pick}, candidates {cands}")
        print(lines[-1], flush=True)
        rows = B * D
        x = torch.randn(B, D, T, device=DEV, dtype=dtype)
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        xr = x.reshape(rows, T, 1)
        nbytes = 2 * rows * T * esz
        variants, plans, outs = {}, {}, {}
        for n in cands:
            plans[n] = mf.plan_fftconv(dtype, B, D, T, n, taps=K)
            plans[n].set_filter(k)
            outs[n] = torch.empty(plans[n].out_shape, device=DEV, dtype=dtype)
            variants[f"fused{n}"] = (lambda p, o: lambda: mf.fft(o, xr, ctx, plan=p))(plans[n], outs[n])
        # (b) at the picked block
        S = pick - K + 1
        F = -(-T // S)
        single = mf.plan_fftconv(dtype, B * F, D, pick, pick, offset=K - 1, out_length=S)
        single.set_filter(k)
        yb = torch.empty(single.out_shape, device=DEV, dtype=dtype)

        def composition():
            xb = blocks_of(x, pick, K)
            mf.fft(yb, xb.reshape(B * F * D, pick, 1), ctx, plan=single)
            return rows_of(yb.reshape(B, F, D, S), T)

        variants["composition"] = composition
        # (c) torch.fft at the full length
        m = scipy.fft.next_fast_len(T + K - 1, real=True)
        torch_note = f"torch.fft.rfft / irfft at {m} points, product and crop included"
        try:
            Hfull = torch.fft.rfft(k, m)

            def full_fft():
                return torch.fft.irfft(torch.fft.rfft(x, m) * Hfull, m)[..., :T].contiguous()

            full_fft()  # (runs it once: a failure shows here, not in the windows)
            err_c = None
            variants["torchfft"] = full_fft
        except Exception as e:  # (reported as what it is: yardstick (c) is then missing for this shape)
            torch_note = f"torch.fft failed at {m} points: {type(e).__name__}: {str(e).splitlines()[0][:120]}"
            err_c = None
        src = torch.empty(rows * T, device=DEV, dtype=dtype).normal_()
        dst = torch.empty_like(src)
        variants["copy"] = lambda: dst.copy_(src)
        # agreement before any timing
        mf.fft(outs[pick], xr, ctx, plan=plans[pick])
        ref = composition().reshape(rows, T)
        err = ((ref - outs[pick].reshape(rows, T)).norm() / ref.norm()).item()
        if "torchfft" in variants:
            err_c = ((variants["torchfft"]().reshape(rows, T) - ref).norm() / ref.norm()).item()
        del ref
        t = measure(variants)
        for n in cands:
            p = plans[n]
            report(lines, f"(a) fused, block {n}" + (" (picked)" if n == pick else ""), t[f"fused{n}"], nbytes,
                   f"{p.kernel_name(1)} geometry={p.pass_geometry(1)} blocks per row {p.blocks} step {p.step}")
        report(lines, f"(b) composition, block {pick}", t["composition"], nbytes,
               f"pad + unfold.contiguous + {single.kernel_name(1)} + reshape + crop (agrees with (a) to {err:.1e})")
        if "torchfft" in t:
            report(lines, "(c) torch.fft, full length", t["torchfft"], nbytes, torch_note + f" (agrees with (b) to {err_c:.1e})")
        else:
            lines.append(f"  (c) {torch_note}")
            print(lines[-1], flush=True)
        report(lines, "(d) copy of (a)'s bytes", t["copy"], nbytes, "torch copy_ of nbytes / 2: read + written = nbytes")
        a, b = t[f"fused{pick}"], t["composition"]
        met = a[0] <= b[0] + (b[2] - b[1])
        fastest = min(cands, key=lambda n: t[f"fused{n}"][0])
        lines.append(f"  ratios: (a) / (b) {ratio(a, b)}   (a) / (d) {ratio(a, t['copy'])}" +
                     (f"   (a) / (c) {ratio(a, t['torchfft'])}" if "torchfft" in t else ""))
        print(lines[-1], flush=True)
        lines.append(f"  condition: {a[0]:.4f} <= {b[0]:.4f} + {b[2] - b[1]:.4f}: {'met' if met else 'MISSED'}")
        print(lines[-1], flush=True)
        lines.append(f"  fftconv_block's rule picked {pick}; the fastest candidate by median was {fastest}" +
                     ("" if fastest == pick else f" ((a, {pick}) / (a, {fastest}) {ratio(a, t[f'fused{fastest}'])})"))
        print(lines[-1], flush=True)
        del x, k, xr, plans, outs, single, yb, src, dst, variants
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    for dtype in (torch.float32, torch.float64):
        B, D, T, K = 32, 1, 480000, 33
        tname = "fp32" if dtype == torch.float32 else "fp64"
        sizes = [256 << i for i in range(7) if 256 << i <= (8192 if dtype == torch.float64 else 16384)]
        lines.append(f"sweep {B}x{D}x{T} K={K} {tname}: fused plans at every block length; per block sample = median * S / n")
        print(lines[-1], flush=True)
        x = torch.randn(B, D, T, device=DEV, dtype=dtype)
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        xr = x.reshape(B * D, T, 1)
        plans = {n: mf.plan_fftconv(dtype, B, D, T, n, taps=K) for n in sizes}
        outs = {n: torch.empty(plans[n].out_shape, device=DEV, dtype=dtype) for n in sizes}
        for p in plans.values():
            p.set_filter(k)
        t = measure({n: (lambda p, o: lambda: mf.fft(o, xr, ctx, plan=p))(plans[n], outs[n]) for n in sizes})
        per = {n: t[n][0] * plans[n].step / n for n in sizes}
        best = min(per.values())
        for n in sizes:
            report(lines, f"block {n}", t[n], 2 * B * D * T * (4 if dtype == torch.float32 else 8),
                   f"{plans[n].kernel_name(1)} geometry={plans[n].pass_geometry(1)} per block sample {per[n]:.4f} ms = "
                   f"{per[n] / best:.2f} x the cheapest")
        del x, k, xr, plans, outs
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
