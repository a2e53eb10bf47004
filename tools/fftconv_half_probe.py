"""Half-storage fftconv (mf.plan_fftconv(torch.float32, ..., io_dtype=torch.bfloat16); bits 8..15 of the MIFFT_CONV_TAG mode
word) beside its yardsticks, in one process per run, at the shapes of profiles/r18_fftconv_gate.txt and one partitioned shape,
ungated and with both gates:
  (h) the half-storage plan: bfloat16 x (and gates) in, bfloat16 y out, one launch;
  (a) the composition it replaces: x.float() (and the gates' .float()), the float32 plan of the same shape, y.to(bfloat16) --
      one widening launch per tensor, one narrowing launch and 4-byte intermediates from torch's caching allocator, as a
      caller under autocast has them.  THE CONDITION: (h) is not slower than (a) beyond the spread of (a)'s own windows;
  (b) the float32 plan of the same shape alone, on float32 tensors: reported, not conditioned (the LDS passes bind these
      kernels, not HBM: no factor of two is expected).
Before any timing (h) is compared with (a) bit for bit.  The backward, reported only: loss.backward() through
mf.fftconv(..., io_dtype=torch.bfloat16) beside torch autograd over the widened composition
mf.fftconv(x.float(), k, pregate=a.float(), postgate=b.float()).to(torch.bfloat16), forward included in both.
Timing: HIP events around windows of CALLS calls (backward: CALLS_BWD), the variants of a shape alternating window by window
inside the process, WARM warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
Bytes are each variant's own compulsory traffic -- every tensor moved once, 2 bytes per element for (h), 4 for (b); (a) is
charged (h)'s bytes: what the caller holds.
    python tools/fftconv_half_probe.py [out.txt]        (default: profiles/r21_fftconv_half.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L, K, n, taps, partition)
SHAPES = [(8, 768, 8192, 8192, 16384, None, None), (64, 256, 1024, 1024, 2048, None, None),
          (32, 1, 480000, 257, 4096, 257, None), (32, 1, 480000, 4097, 16384, 4097, None),
          (4, 256, 32768, 32768, 16384, 32768, 8193)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, CALLS_BWD, WARM = 7, 20, 4, 3
DEV = "cuda:0"
IO = torch.bfloat16


def measure(variants, calls):
    """{name: fn} -> {name: (median ms, min ms, max ms)}: windows of ``calls`` calls, the variants alternating"""
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def report(lines, label, t, nbytes, note):
    med, lo, hi = t
    frac = nbytes / (med * 1e-3) / PEAK
    lines.append(f"  {label:<34} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {note}")
    print(lines[-1], flush=True)


def ratio(a, b):
    """median a / median b with the spread the run shows: [min a / max b .. max a / min b]"""
    return f"{a[0] / b[0]:.3f} [{a[1] / b[2]:.3f} .. {a[2] / b[1]:.3f}]"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_fftconv_half.txt")
    lines = [f"# tools/fftconv_half_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (backward: {CALLS_BWD}; HIP events), variants alternating, {WARM} warm-up calls each",
             "# (h) half-storage plan, bfloat16 in and out; (a) widen + float32 plan + narrow; (b) float32 plan alone on float32 tensors",
             "# bytes: every tensor of the variant once (gates 3: x, a, y, b; gates 0: x, y), 2 bytes per element for (h) and (a), 4 for (b)",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median (h) <= median (a) + (max (a) - min (a))"]
    ctx = mf.DeviceContext(0)
    for B, D, L, K, n, taps, Q in SHAPES:
        kind = "partitioned" if Q else "overlap-save" if taps else "single block"
        rows = B * D
        k = torch.randn(D, K, device=DEV) / K ** 0.5
        xh, ah, bh = (torch.randn(rows, L, 1, device=DEV).to(IO) for _ in range(3))
        xf, af, bf = xh.float(), ah.float(), bh.float()
        for gates in (0, 3):
            lines.append(f"{B}x{D}x{L} K={K} n={n} {kind}" + (f" Q={Q}" if Q else "") + f" gates={gates} bfloat16")
            print(lines[-1], flush=True)
            kw = dict(taps=taps, partition=Q, pregate=bool(gates & 1), postgate=bool(gates & 2))
            hp = mf.plan_fftconv(torch.float32, B, D, L, n, io_dtype=IO, **kw)
            fp = mf.plan_fftconv(torch.float32, B, D, L, n, **kw)
            hp.set_filter(k)
            fp.set_filter(k)
            yh = torch.empty(hp.out_shape, device=DEV, dtype=IO)
            yf = torch.empty(fp.out_shape, device=DEV)
            ya = torch.empty(fp.out_shape, device=DEV)

            if gates:
                half = lambda: hp.run(yh, xh, pregate=ah, postgate=bh)
                plain = lambda: fp.run(yf, xf, pregate=af, postgate=bf)

                def composition():
                    fp.run(ya, xh.float(), pregate=ah.float(), postgate=bh.float())
                    return ya.to(IO)
            else:
                half = lambda: mf.fft(yh, xh, ctx, plan=hp)
                plain = lambda: mf.fft(yf, xf, ctx, plan=fp)

                def composition():
                    mf.fft(ya, xh.float(), ctx, plan=fp)
                    return ya.to(IO)

            half()
            same = bool(torch.equal(yh.view(torch.int16), composition().view(torch.int16)))
            t = measure({"half": half, "composition": composition, "float32": plain}, CALLS)
            one = rows * L * 2
            tensors = 4 if gates else 2
            geo = f"geometry={hp.pass_geometry(1)}" + (f" blocks per row {hp.blocks} step {hp.step}" if taps else "")
            report(lines, "(h) half-storage plan", t["half"], tensors * one, f"{hp.kernel_name(1)} {geo}")
            report(lines, "(a) widen + float32 + narrow", t["composition"], tensors * one,
                   f"{tensors - 1} x .float() + {fp.kernel_name(1)} + .to(bfloat16) ((h) equals it bit for bit: {same})")
            report(lines, "(b) float32 plan alone", t["float32"], 2 * tensors * one, fp.kernel_name(1))
            th, ta, tb = t["half"], t["composition"], t["float32"]
            met = th[0] <= ta[0] + (ta[2] - ta[1])
            lines.append(f"  ratios: (h) / (a) {ratio(th, ta)}   (h) / (b) {ratio(th, tb)}")
            print(lines[-1], flush=True)
            lines.append(f"  condition: {th[0]:.4f} <= {ta[0]:.4f} + {ta[2] - ta[1]:.4f}: {'met' if met else 'MISSED'}")
            print(lines[-1], flush=True)
            del hp, fp, yh, yf, ya
        # the backward (gates 3), reported only; the partitioned shape's filter gradient is one launch per partition
        sel = dict(block=n, partition=Q) if Q else dict(block=n) if taps else dict(n=n)
        shape = (B, D, L)
        leaves = lambda dt: [v.reshape(shape).to(dt).clone().requires_grad_(True) for v in (xh, ah, bh)]
        kk = k.clone().requires_grad_(True)
        hx, ha, hb = leaves(IO)
        wx, wa, wb = leaves(IO)
        gy = torch.randn(shape, device=DEV).to(IO)

        def bwd_half():
            mf.fftconv(hx, kk, pregate=ha, postgate=hb, io_dtype=IO, **sel).backward(gy)
            hx.grad = ha.grad = hb.grad = kk.grad = None

        def bwd_composition():
            mf.fftconv(wx.float(), kk, pregate=wa.float(), postgate=wb.float(), **sel).to(IO).backward(gy)
            wx.grad = wa.grad = wb.grad = kk.grad = None

        t = measure({"half": bwd_half, "composition": bwd_composition}, CALLS_BWD)
        lines.append(f"{B}x{D}x{L} K={K} n={n} {kind} gates=3 bfloat16, forward + backward of x, k, both gates")
        print(lines[-1], flush=True)
        report(lines, "(h) io_dtype=bfloat16", t["half"], 0, "mf.fftconv(..., io_dtype=torch.bfloat16) and its backward")
        report(lines, "(a) autograd over the widened", t["composition"], 0, "mf.fftconv(x.float(), ...).to(bfloat16) and torch's casts in the graph")
        lines.append(f"  ratio: (h) / (a) {ratio(t['half'], t['composition'])}   (reported, not conditioned)")
        print(lines[-1], flush=True)
        del xh, ah, bh, xf, af, bf, k, kk, hx, ha, hb, wx, wa, wb, gy
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
