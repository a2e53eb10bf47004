"""Partitioned fftconv (mf.plan_fftconv(taps=K, partition=Q); TileCfg::PART, the 20-word MIFFT_CONV_TAG payload) beside its
yardsticks, in one process per run, with a causal filter as long as the row (K = L) at fftconv_partition's (n, Q):
  the plan: one launch of the partitioned plan (forward), and the whole backward of mf.fftconv(x, k, partition=Q) with x and k
      wanting gradients (one launch of the opposite-correlate partitioned plan, one overlap-save filter-gradient launch per
      partition).
  (a) the composition that gave the same result before: P overlap-save launches at taps = Q, partition p on the same rows with
      L - p Q samples stored, plus the P - 1 adds of those into y[..., p Q:] (forward); its backward by torch autograd over the
      differentiable overlap-save mf.fftconv(block=n) of every partition, shifted with a pad.
  (b) torch.fft.rfft / irfft at one full length (the power of two from 2 L on), forward, and backward by torch autograd.
  (c) the overlap-save plan at K = 8193 (fp64: 4097) taps on the same rows: what one partition costs, forward only.
Before any timing the plan is compared with (a) (the worst row's relative l2), and with (b).
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition printed per shape, forward and backward: the plan's median is not above (a)'s by more than the spread
(max - min) of (a)'s own windows.
    python tools/fftconv_part_probe.py [out.txt]        (default: profiles/r20_fftconv_part.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (B, D, L = K, dtype)
SHAPES = [(4, 256, 32768, torch.float32), (4, 256, 65536, torch.float32), (4, 64, 131072, torch.float32),
          (4, 64, 32768, torch.float64)]
WINDOWS, CALLS, WARM = 7, 3, 1
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


def worst(got, ref):
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max())


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_fftconv_part.txt")
    lines = [f"# tools/fftconv_part_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up call(s) each",
             "# causal, K = L, (n, Q) = fftconv_partition(K); ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median (plan) <= median (a) + (max - min of (a)'s windows), forward and backward"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<58} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    pad = torch.nn.functional.pad
    for B, D, L, dtype in SHAPES:
        K = L
        n, Q = mf.fftconv_partition(K, dtype)
        P = -(-K // Q)
        rows = B * D
        say(f"{B}x{D}x{L} K={K} n={n} Q={Q} P={P} {'fp32' if dtype == torch.float32 else 'fp64'}")
        x = torch.randn(B, D, L, device=DEV, dtype=dtype)
        k = torch.randn(D, K, device=DEV, dtype=dtype) / K ** 0.5
        gy = torch.randn(B, D, L, device=DEV, dtype=dtype)
        xr = x.reshape(rows, L, 1)
        plan = mf.plan_fftconv(dtype, B, D, L, n, taps=K, partition=Q)
        plan.set_filter(k)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        # (a): partition p is an overlap-save plan of Q taps on the same rows that stores the first L - p Q samples
        parts = []
        for p in range(P):
            if L - p * Q < 1:
                break
            q = mf.plan_fftconv(dtype, B, D, L, n, taps=Q, out_length=L - p * Q)
            q.set_filter(k[:, p * Q:(p + 1) * Q])
            parts.append((p, q, torch.empty(q.out_shape, device=DEV, dtype=dtype)))
        ya = torch.empty(rows, L, 1, device=DEV, dtype=dtype)

        def composed():
            for p, q, o in parts:
                mf.fft(ya if p == 0 else o, xr, plan=q)
                if p:
                    ya[:, p * Q:] += o
            return ya

        nfft = 1 << (2 * L - 1).bit_length()

        def torch_fft(x, k):
            return torch.fft.irfft(torch.fft.rfft(x, n=nfft) * torch.fft.rfft(k, n=nfft), n=nfft)[..., :L]

        Kc = Q
        one = mf.plan_fftconv(dtype, B, D, L, n, taps=Kc)
        one.set_filter(k[:, :Kc])
        out_c = torch.empty(one.out_shape, device=DEV, dtype=dtype)
        mf.fft(out, xr, plan=plan)
        err_a, err_b = worst(out[..., 0], composed()[..., 0]), worst(out.reshape(B, D, L), torch_fft(x, k))
        say(f"  worst row rel l2 of the plan against (a) {err_a:.2e}, against (b) {err_b:.2e}")
        # backward: x and k want gradients; the forward graphs are built once, the backward timed
        xs, ks = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
        y_mf = mf.fftconv(xs, ks, block=n, partition=Q)
        y_a = None
        for p in range(P):
            if L - p * Q < 1:
                break
            yp = mf.fftconv(xs, ks[:, p * Q:(p + 1) * Q], block=n)
            y_a = yp if p == 0 else y_a + pad(yp[..., :L - p * Q], (p * Q, 0))
        y_b = torch_fft(xs, ks)
        g_mf, g_a = torch.autograd.grad(y_mf, (xs, ks), gy, retain_graph=True), torch.autograd.grad(y_a, (xs, ks), gy, retain_graph=True)
        say(f"  backward of the plan against (a)'s: gx {worst(g_mf[0], g_a[0]):.2e}, gk {worst(g_mf[1], g_a[1]):.2e}")
        del g_mf, g_a
        variants = {"plan": lambda: mf.fft(out, xr, plan=plan), "a": composed, "b": lambda: torch_fft(x, k),
                    "c": lambda: mf.fft(out_c, xr, plan=one),
                    "plan bwd": lambda: torch.autograd.grad(y_mf, (xs, ks), gy, retain_graph=True),
                    "a bwd": lambda: torch.autograd.grad(y_a, (xs, ks), gy, retain_graph=True),
                    "b bwd": lambda: torch.autograd.grad(y_b, (xs, ks), gy, retain_graph=True)}
        t = measure(variants)
        row("the partitioned plan, forward", t["plan"], f"{plan.kernel_name(1)} geometry={plan.pass_geometry(1)} blocks {plan.blocks}")
        row(f"(a) {len(parts)} overlap-save launches + adds, forward", t["a"])
        row(f"(b) torch.fft at {nfft} points, forward", t["b"])
        row(f"(c) one overlap-save plan of {Kc} taps, forward", t["c"])
        row("the partitioned backward (gx, gk)", t["plan bwd"])
        row("(a) backward by autograd over the overlap-save launches", t["a bwd"])
        row("(b) backward by autograd over torch.fft", t["b bwd"])
        say(f"  ratios forward: plan / (a) {ratio(t['plan'], t['a'])}   plan / (b) {ratio(t['plan'], t['b'])}   "
            f"plan / (c) {ratio(t['plan'], t['c'])}")
        say(f"  ratios backward: plan / (a) {ratio(t['plan bwd'], t['a bwd'])}   plan / (b) {ratio(t['plan bwd'], t['b bwd'])}")
        for what, ta, tb in (("forward", t["plan"], t["a"]), ("backward", t["plan bwd"], t["a bwd"])):
            met = ta[0] <= tb[0] + (tb[2] - tb[1])
            say(f"  condition {what}: {ta[0]:.4f} <= {tb[0]:.4f} + {tb[2] - tb[1]:.4f}: {'met' if met else 'MISSED'}")
        del x, k, gy, xr, out, parts, ya, out_c, xs, ks, y_mf, y_a, y_b, variants, plan, one
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
