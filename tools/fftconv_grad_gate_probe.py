"""Gates fused into the filter gradient of fftconv (mf.plan_fftconv_grad(pregate=True, postgate=True); TileCfg::WGRAD with
TileCfg::GATE, word 11 of the MIFFT_CONV_GRAD_TAG payload) beside what they replace, in one process per run, at the shapes of
profiles/r19_fftconv_grad.txt:
  fused   the gated plan's filter_grad on (x, gy, a, b): the kernel with both gates in its loads, the sum of its partials, the
          irfftn of the channels' rows.  Also with the pregate alone.
  (a)     the composition it replaces, in the same build: the two torch products u = a * x and gv = b * gy -- on 16-bit rows
          the widening products a.float() * x.float() and b.float() * gy.float(), as the backward of mf.fftconv formed them --
          and the ungated plan's filter_grad on them (16-bit rows: the float32 plan).  With the pregate alone: one product
          (16-bit rows: and gy.float()).
  (b)     the ungated plan's filter_grad alone, on products formed before the clock starts.
  backward  the whole backward of the gated op (x, k, pregate, postgate, skip all wanting gradients) through mf.fftconv's
          autograd.Function against the same backward by torch autograd over torch.fft (16-bit rows: over the widened tensors).
Before any timing the fused result is compared with (a)'s bit for bit.
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition printed per shape and gate set: the fused median is not above (a)'s by more than the spread (max - min) of (a)'s
own windows.
    python tools/fftconv_grad_gate_probe.py [out.txt]        (default: profiles/r22_fftconv_grad_gate.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L, K, n, overlap-save, the plan's dtype, io_dtype)
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SHAPES = [(8, 768, 8192, 8192, 16384, False, F32, None), (8, 768, 8192, 8192, 16384, False, F32, BF16),
          (64, 256, 1024, 1024, 2048, False, F32, None), (64, 256, 1024, 1024, 2048, False, F64, None),
          (32, 1, 480000, 257, 4096, True, F32, None), (32, 1, 480000, 4097, 16384, True, F32, None)]
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_fftconv_grad_gate.txt")
    lines = [f"# tools/fftconv_grad_gate_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of "
             f"{CALLS} calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# fused: the gated plan's filter_grad (kernel + sum of partials + irfftn); (a): the torch products (16-bit rows: the",
             "# widening products) + the ungated plan's filter_grad; (b): the ungated plan's filter_grad on products formed beforehand",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median fused <= median (a) + (max - min of (a)'s windows)"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<58} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    for B, D, L, K, n, ols, dtype, io in SHAPES:
        sdt = io or dtype
        tname = {F32: "fp32", F64: "fp64"}[dtype] + (" bf16 rows" if io is not None else "")
        say(f"{B}x{D}x{L} K={K} n={n} {'overlap-save' if ols else 'single block'} {tname}")
        taps = K if ols else None
        x, gy, a, b = (torch.randn(B, D, L, device=DEV, dtype=torch.float32).to(sdt) for _ in range(4))
        both = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=taps, io_dtype=io, pregate=True, postgate=True)
        pre = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=taps, io_dtype=io, pregate=True)
        plain = mf.plan_fftconv_grad(dtype, B, D, L, n, taps=taps)  # (what (a) and (b) run: the plan's own float type)
        xr, ar = x.reshape(both.in_shape), a.reshape(both.in_shape)
        gr, br = gy.reshape(both.grad_shape), b.reshape(both.grad_shape)
        wide = (lambda t: t.float()) if io is not None else (lambda t: t)

        def comp3():
            return plain.filter_grad(wide(ar) * wide(xr), wide(br) * wide(gr), K)

        def comp1():
            return plain.filter_grad(wide(ar) * wide(xr), wide(gr), K)

        u, gv = wide(ar) * wide(xr), wide(br) * wide(gr)
        same3 = torch.equal(both.filter_grad(xr, gr, K, pregate=ar, postgate=br), comp3())
        same1 = torch.equal(pre.filter_grad(xr, gr, K, pregate=ar), comp1())
        say(f"  fused equals (a) bit for bit: both gates {same3}, pregate alone {same1}   {both.kernel_name(1)} partials={both.partials} "
            f"geometry={both.pass_geometry(1)}")
        variants = {"fused3": lambda: both.filter_grad(xr, gr, K, pregate=ar, postgate=br), "comp3": comp3,
                    "fused1": lambda: pre.filter_grad(xr, gr, K, pregate=ar), "comp1": comp1,
                    "alone": lambda: plain.filter_grad(u, gv, K)}
        # the whole backward, all five gradients
        ag, bg = (t.clone().requires_grad_(True) for t in (a, b))
        xs = x.clone().requires_grad_(True)
        k = (torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5).requires_grad_(True)
        d = torch.randn(D, device=DEV, dtype=dtype).requires_grad_(True)
        ins = (xs, k, ag, bg, d)
        nc = n if not ols else 1 << (L + K - 2).bit_length()  # (the FFT length of the torch composition)
        y_mf = mf.fftconv(xs, k, pregate=ag, postgate=bg, skip=d, io_dtype=io, **({"block": n} if ols else {"n": n}))
        y_th = wide(bg) * torch.fft.irfft(torch.fft.rfft(wide(ag) * wide(xs), n=nc) * (torch.fft.rfft(k, n=nc) + d.reshape(D, 1)), n=nc)[..., :L]
        variants["backward"] = lambda: torch.autograd.grad(y_mf, ins, gy, retain_graph=True)
        variants["backward composed"] = lambda: torch.autograd.grad(y_th, ins, wide(gy), retain_graph=True)
        t = measure(variants)
        row("fused, both gates", t["fused3"])
        row("(a) two torch products + the ungated plan", t["comp3"])
        row("fused, pregate alone", t["fused1"])
        row("(a) one torch product + the ungated plan", t["comp1"])
        row("(b) the ungated plan alone on pre-formed products", t["alone"], plain.kernel_name(1))
        row("backward of the gated op, five gradients", t["backward"])
        row("the same backward by torch autograd on torch.fft", t["backward composed"], f"at n = {nc}")
        for name, f, c in (("both gates", "fused3", "comp3"), ("pregate alone", "fused1", "comp1")):
            tf, tc = t[f], t[c]
            met = tf[0] <= tc[0] + (tc[2] - tc[1])
            say(f"  {name}: fused / (a) {ratio(tf, tc)}   fused / (b) {ratio(tf, t['alone'])}")
            say(f"  {name}: condition {tf[0]:.4f} <= {tc[0]:.4f} + {tc[2] - tc[1]:.4f}: {'met' if met else 'MISSED'}")
        say(f"  backward / backward composed {ratio(t['backward'], t['backward composed'])}")
        del x, gy, a, b, xr, ar, gr, br, u, gv, ag, bg, xs, k, d, ins, y_mf, y_th, variants, both, pre, plain
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
