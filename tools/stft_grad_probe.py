"""The backward of mf.stft and of the power-2 mf.spectrogram (the fused adjoint overlap-add: mf.plan_stft_adjoint, the ISTFT tile
with TileCfg::ADJ) beside what it replaces, in one process per run; fp32, centred reflect, Hann window:
  stft bwd   torch.autograd.grad over mf.stft: one adjoint launch in mode 1 and the fold of the two edge strips.
  spec bwd   the same over mf.spectrogram(power=2): one stft launch that recomputes X, one adjoint launch in mode 2, the fold.
  (a)        torch.autograd over torch.stft (for the spectrogram: .abs().pow(2)) on the same tensors.
  (b)        the same adjoint composed in this build: mf.stft, the torch product (2 m)[..., None] * X, the mode-1 plan's apply.
  (c)        the plan_istft launch over the same frames: the floor for the store (it divides by the envelope besides).
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.  No condition on speed.
    python tools/stft_grad_probe.py [out.txt]        (default: profiles/r23_stft_grad.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

SHAPES = [(32, 480000, 400, 160), (32, 220500, 1024, 256)]  # (B, T, n_fft, hop)
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_stft_grad.txt")
    lines = [f"# tools/stft_grad_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each; fp32, centre reflect, Hann window",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]; no condition on speed"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<64} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    for B, T, n, hop in SHAPES:
        say(f"{B} x {T}, n_fft {n} / hop {hop}")
        w = torch.hann_window(n, dtype=torch.float32, device=DEV)
        x = torch.randn(B, T, device=DEV).requires_grad_()
        X_mf = mf.stft(x, n, hop, window=w)
        P_mf = mf.spectrogram(x, n, hop, window=w, power=2)
        X_th = torch.stft(x, n, hop, window=w, center=True, pad_mode="reflect", return_complex=True)
        P_th = X_th.abs().pow(2)
        gX, gP = torch.randn_like(X_mf), torch.randn_like(P_mf)
        adj1 = mf.plan_stft_adjoint(torch.float32, B, T, n, hop, window=w, center="reflect")
        inv = mf.plan_istft(torch.float32, B, adj1.frames, n, hop, window=w, center=True)
        gf = torch.view_as_real(gX.transpose(-1, -2).contiguous()).reshape(adj1.in_shape)
        m = gP.transpose(-1, -2).contiguous()
        sig = torch.empty(inv.out_shape, device=DEV)
        xd = x.detach()

        def composed():
            Xf = torch.view_as_real(mf.stft(xd, n, hop, window=w).transpose(-1, -2)).reshape(adj1.in_shape)
            return adj1.apply((2 * m)[..., None] * Xf)

        got = torch.autograd.grad(P_mf, x, gP, retain_graph=True)[0]
        ref = torch.autograd.grad(P_th, x, gP, retain_graph=True)[0]
        say(f"  spec bwd against (a): max abs difference {float((got - ref).abs().max()):.3e} at max abs {float(ref.abs().max()):.3e}; "
            f"against (b): equal bit for bit {torch.equal(got, composed())}   {adj1.kernel_name(2)} geometry={adj1.pass_geometry(2)}")
        t = measure({
            "stft": lambda: torch.autograd.grad(X_mf, x, gX, retain_graph=True),
            "stft torch": lambda: torch.autograd.grad(X_th, x, gX, retain_graph=True),
            "spec": lambda: torch.autograd.grad(P_mf, x, gP, retain_graph=True),
            "spec torch": lambda: torch.autograd.grad(P_th, x, gP, retain_graph=True),
            "spec composed": composed,
            "istft": lambda: mf.fft(sig, gf, plan=inv),
        })
        row("stft bwd: the adjoint launch (mode 1) + fold", t["stft"])
        row("(a) torch.autograd over torch.stft", t["stft torch"])
        row("spec bwd: stft launch + adjoint launch (mode 2) + fold", t["spec"])
        row("(a) torch.autograd over torch.stft(...).abs().pow(2)", t["spec torch"])
        row("(b) mf.stft, the torch product, the mode-1 plan", t["spec composed"])
        row("(c) the plan_istft launch over the same frames", t["istft"], inv.kernel_name(2))
        say(f"  stft bwd / (a) {ratio(t['stft'], t['stft torch'])}   stft bwd / (c) {ratio(t['stft'], t['istft'])}")
        say(f"  spec bwd / (a) {ratio(t['spec'], t['spec torch'])}   spec bwd / (b) {ratio(t['spec'], t['spec composed'])}")
        del x, X_mf, P_mf, X_th, P_th, gX, gP, gf, m, sig, xd, adj1, inv
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
