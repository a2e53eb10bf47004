"""The fused partitioned filter gradient (mf.plan_fftconv_grad(taps=K, partition=Q, fused=True): FusedPartConvGradPlan -- stage 1
TileCfg::WSPEC, stage 2 lag_corr.hip) beside its yardsticks, in one process per run, with a causal filter as long as the row
(K = L) at fftconv_partition's (n, Q), on the shapes of profiles/r20_fftconv_part.txt:
  fused: FusedPartConvGradPlan.filter_grad at the default scratch limit, and at 64 MiB, at two batch entries per slab and
      unbounded (the sweep; a limit below one batch entry's spectra is refused and reported so).
  (a) PartConvGradPlan.filter_grad (fused=False: one overlap-save filter-gradient launch per partition) on the same tensors.
  (b) the gk part of torch.autograd over torch.fft.rfft / irfft at one full length (the power of two from 2 L on).
  (c) stage 1 alone (the two spectra launches of every slab) and a device copy of as many bytes as the scratch holds: what binds.
  and the whole backward (gx and gk) of mf.fftconv(x, k, partition=Q) with the selector forced to fused and to composed, beside
  torch's.
The second shape runs again in bfloat16 with both gates.  Before any timing the fused result is compared with (a) and with (b)
(the worst row's relative l2).
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition printed per shape -- what _FFTCONV_FUSED_GRAD in api.py records per (storage dtype, n): the fused median is not
above (a)'s by more than the spread (max - min) of (a)'s own windows.
    python tools/fftconv_part_grad_probe.py [out.txt]        (default: profiles/r26_fftconv_part_grad.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L = K, dtype, io_dtype, gated)
SHAPES = [(4, 256, 32768, torch.float32, None, False), (4, 256, 65536, torch.float32, None, False),
          (4, 64, 131072, torch.float32, None, False), (4, 64, 32768, torch.float64, None, False),
          (4, 256, 65536, torch.float32, torch.bfloat16, True)]
WINDOWS, CALLS, WARM = 7, 3, 1
DEV = "cuda:0"
NAMES = {torch.float32: "fp32", torch.float64: "fp64", torch.bfloat16: "bf16", torch.float16: "fp16"}


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


def worst(got, ref):
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max())


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r26_fftconv_part_grad.txt")
    lines = [f"# tools/fftconv_part_grad_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of "
             f"{CALLS} calls (HIP events), variants alternating, {WARM} warm-up call(s) each",
             "# causal, K = L, (n, Q) = fftconv_partition(K); ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition (per storage dtype and n): median (fused) <= median (a) + (max - min of (a)'s windows)"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<66} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    for B, D, L, dtype, io, gated in SHAPES:
        K = L
        n, Q = mf.fftconv_partition(K, dtype)
        rows, sdt = B * D, io or dtype
        say(f"{B}x{D}x{L} K={K} n={n} Q={Q} {NAMES[sdt]}{' pregate postgate' if gated else ''}")
        x = torch.randn(B, D, L, device=DEV, dtype=torch.float32).to(sdt)
        gy = torch.randn(B, D, L, device=DEV, dtype=torch.float32).to(sdt)
        a = torch.randn(B, D, L, device=DEV, dtype=torch.float32).to(sdt) if gated else None
        b = torch.randn(B, D, L, device=DEV, dtype=torch.float32).to(sdt) if gated else None
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        r3 = lambda t: None if t is None else t.reshape(rows, L, 1)
        xr, gr, ar, br = r3(x), r3(gy), r3(a), r3(b)
        gates = dict(pregate=ar, postgate=br) if gated else {}
        kw = dict(taps=K, partition=Q, io_dtype=io, pregate=gated, postgate=gated)
        fused = mf.plan_fftconv_grad(dtype, B, D, L, n, fused=True, **kw)
        composed = mf.plan_fftconv_grad(dtype, B, D, L, n, **kw)
        unbounded = mf.plan_fftconv_grad(dtype, B, D, L, n, fused=True, scratch_bytes=1 << 60, **kw)
        try:
            small = mf.plan_fftconv_grad(dtype, B, D, L, n, fused=True, scratch_bytes=64 << 20, **kw)
        except mf.MifftError:
            small = None  # (one batch entry's spectra are above 64 MiB)
        two = mf.plan_fftconv_grad(dtype, B, D, L, n, fused=True, scratch_bytes=2 * fused.entry_bytes, **kw)
        g = fused.geometry
        say(f"  hop {fused.hop}, {fused.lag_groups} lag groups, {g.Fu} live u-frames + {g.Fg} g-blocks per row; the composed plan: "
            f"{composed.num_launches} launches; one entry's spectra {fused.entry_bytes / 2 ** 20:.1f} MiB")
        nfft = 1 << (2 * L - 1).bit_length()
        wide = lambda t: t.to(dtype)
        u, gv = (wide(x) * wide(a), wide(gy) * wide(b)) if gated else (wide(x), wide(gy))

        def torch_fft(x, k):
            return torch.fft.irfft(torch.fft.rfft(x, n=nfft) * torch.fft.rfft(k, n=nfft), n=nfft)[..., :L]

        ks = k.clone().requires_grad_(True)
        y_b = torch_fft(u, ks)
        got = fused.filter_grad(xr, gr, K, **gates)
        err_a = worst(got, composed.filter_grad(xr, gr, K, **gates))
        err_b = worst(got, torch.autograd.grad(y_b, ks, gv, retain_graph=True)[0])
        say(f"  worst row rel l2 of the fused gradient against (a) {err_a:.2e}, against (b) {err_b:.2e}")
        spare = torch.empty(unbounded.scratch_bytes // 4, device=DEV, dtype=torch.float32)
        src = torch.empty_like(spare)

        def stage1():
            for i in range(len(unbounded.slabs)):
                unbounded.spectra(xr, gr, i, **gates)

        variants = {"fused": lambda: fused.filter_grad(xr, gr, K, **gates), "a": lambda: composed.filter_grad(xr, gr, K, **gates),
                    "b": lambda: torch.autograd.grad(y_b, ks, gv, retain_graph=True),
                    "unbounded": lambda: unbounded.filter_grad(xr, gr, K, **gates), "stage1": stage1,
                    "copy": lambda: spare.copy_(src)}
        if small is not None:
            variants["64MiB"] = lambda: small.filter_grad(xr, gr, K, **gates)
        variants["two"] = lambda: two.filter_grad(xr, gr, K, **gates)
        t = measure(variants)
        row(f"fused, default limit: {len(fused.slabs)} slab(s), scratch {fused.scratch_bytes / 2 ** 20:.0f} MiB", t["fused"],
            f"{fused.plans[0][0].kernel_name(1)} {fused.plans[0][1].kernel_name(1)} {fused.plans[0][2].kernel_name(1)}")
        if small is not None:
            row(f"fused, 64 MiB: {len(small.slabs)} slab(s), scratch {small.scratch_bytes / 2 ** 20:.0f} MiB", t["64MiB"])
        else:
            say("  fused, 64 MiB: refused (one batch entry's spectra are larger)")
        row(f"fused, two entries: {len(two.slabs)} slab(s), scratch {two.scratch_bytes / 2 ** 20:.0f} MiB", t["two"])
        row(f"fused, unbounded: {len(unbounded.slabs)} slab(s), scratch {unbounded.scratch_bytes / 2 ** 20:.0f} MiB", t["unbounded"])
        row(f"(a) composed: {composed.num_launches} filter-gradient launches", t["a"])
        row(f"(b) gk of torch.autograd over torch.fft at {nfft} points", t["b"])
        row("(c) stage 1 alone (unbounded plan)", t["stage1"])
        row(f"(c) a copy of {unbounded.scratch_bytes / 2 ** 20:.0f} MiB", t["copy"])
        say(f"  ratios: fused / (a) {ratio(t['fused'], t['a'])}   fused / (b) {ratio(t['fused'], t['b'])}   "
            f"stage 1 / fused(unbounded) {ratio(t['stage1'], t['unbounded'])}")
        met = t["fused"][0] <= t["a"][0] + (t["a"][2] - t["a"][1])
        say(f"  condition ({NAMES[sdt]}, n = {n}): {t['fused'][0]:.4f} <= {t['a'][0]:.4f} + {t['a'][2] - t['a'][1]:.4f}: "
            f"{'met' if met else 'MISSED'}")
        del spare, src, variants, fused, composed, unbounded, small, two
        # the whole backward of mf.fftconv: gx and gk, the selector forced either way, beside torch's
        if not gated:
            xs, kk = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
            with mf.fftconv_fused_filter_grad(True):  # (the forward asks the selector for its backward)
                y_f = mf.fftconv(xs, kk, block=n, partition=Q)
            with mf.fftconv_fused_filter_grad(False):
                y_c = mf.fftconv(xs, kk, block=n, partition=Q)
            y_t = torch_fft(xs, kk)
            bwd = lambda y: torch.autograd.grad(y, (xs, kk), gy, retain_graph=True)
            say(f"  whole backward, fused against composed: gx {worst(bwd(y_f)[0], bwd(y_c)[0]):.2e}, gk {worst(bwd(y_f)[1], bwd(y_c)[1]):.2e}")
            t = measure({"fused": lambda: bwd(y_f), "composed": lambda: bwd(y_c), "torch": lambda: bwd(y_t)})
            row("whole backward (gx, gk), fused filter gradient", t["fused"])
            row("whole backward (gx, gk), composed filter gradient", t["composed"])
            row("whole backward (gx, gk), torch.autograd over torch.fft", t["torch"])
            say(f"  ratios backward: fused / torch {ratio(t['fused'], t['torch'])}   composed / torch {ratio(t['composed'], t['torch'])}")
            del xs, kk, y_f, y_c, y_t
        del x, gy, a, b, k, ks, y_b, u, gv, xr, gr, ar, br, gates
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
