"""The backward of mf.istft (the fused adjoint: mf.plan_istft_adjoint, the STFT tile with TileCfg::IADJ) beside what it replaces,
and the backward of mf.mdct / mf.imdct (each the other's fused plan), in one process per run; centred, Hann window:
  istft bwd  torch.autograd.grad over mf.istft: one adjoint launch on gy.
  (a)        the composition it replaces in this build: gy * (1 / envelope) in torch, mf.stft(center=True, pad_mode="constant",
             window=w) on the product, then the c_k g / n product on the spectrogram-sized result.
  (b)        torch.autograd over torch.istft on the same tensors.
  (c)        the plain plan_stft launch on the same bytes: the floor (it reads no table and halves no bin).
  mdct / imdct bwd   torch.autograd.grad over mf.mdct / mf.imdct at n = 256, beside torch.autograd over a dense cosine-matrix
             composition in torch (frames @ C.T; X @ C and two shifted adds).  Nothing fused is replaced here: report only.
Timing: HIP events around windows of CALLS calls, the variants of a shape alternating window by window inside the process, WARM
warm-up calls each first; the figure is the median of WINDOWS windows, the spread their min .. max.
The condition: istft bwd not slower than (a) beyond the spread of (a)'s own windows -- median(istft bwd) <= median(a) + (max(a) -
min(a)) -- at every shape.
    python tools/istft_grad_probe.py [out.txt]        (default: profiles/r24_istft_grad.txt)"""
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

SHAPES = [(32, 480000, 400, 160, torch.float32), (32, 480000, 1024, 256, torch.float32),
          (32, 480000, 400, 160, torch.float64)]  # (B, T, n_fft, hop, dtype)
MDCT_N = 256
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_istft_grad.txt")
    lines = [f"# tools/istft_grad_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each; centred, Hann window",
             "# ratio p / q = median p / median q [min p / max q .. max p / min q]",
             "# condition: median(istft bwd) <= median(a) + (max(a) - min(a)), at every shape"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def row(label, t, note=""):
        say(f"  {label:<64} {t[0]:9.4f} ms  [{t[1]:.4f} .. {t[2]:.4f}]  {note}")

    met = []
    for B, T, n, hop, dt in SHAPES:
        name = str(dt).replace("torch.", "")
        say(f"{B} x {T}, n_fft {n} / hop {hop}, {name}")
        ct = torch.complex64 if dt == torch.float32 else torch.complex128
        F, c, bins = 1 + T // hop, n // 2, n // 2 + 1
        w = torch.hann_window(n, dtype=dt, device=DEV)
        X = torch.randn(B, bins, F, dtype=ct, device=DEV).transpose(-1, -2).contiguous().transpose(-1, -2).requires_grad_()
        gy = torch.randn(B, T, dtype=dt, device=DEV)
        y_mf = mf.istft(X, n, hop, window=w, length=T)
        y_th = torch.istft(X, n, hop, window=w, length=T)
        # (a): the reciprocal envelope of the stored samples, formed once; c_k / n per bin
        env = torch.zeros(n + hop * (F - 1), dtype=torch.float64, device=DEV)
        w2 = (w.double() ** 2)
        for f0 in range(0, F):
            env[f0 * hop:f0 * hop + n] += w2
        inv_env = (1.0 / env[c:c + T]).to(dt)
        ck = torch.full((bins, 1), 2.0 / n, dtype=dt, device=DEV)
        ck[0] = ck[-1] = 1.0 / n

        def composed():
            return mf.stft(gy * inv_env, n, hop, window=w, center=True, pad_mode="constant") * ck

        adj = mf.plan_istft_adjoint(dt, B, F, n, hop, window=w, center=True, length=T)
        fwd = mf.plan_stft(dt, B, T, n, hop, window=w, center="constant")
        spec = torch.empty(fwd.out_shape, dtype=dt, device=DEV)
        gy3 = gy.reshape(B, T, 1)
        got = torch.autograd.grad(y_mf, X, gy, retain_graph=True)[0]
        ref = torch.autograd.grad(y_th, X, gy, retain_graph=True)[0]
        cmp = composed()
        cmp_d = (got - cmp).abs().max()
        say(f"  istft bwd against (b): max abs difference {float((got - ref).abs().max()):.3e} at max abs {float(ref.abs().max()):.3e}; "
            f"against (a): {float(cmp_d):.3e}   {adj.kernel_name(1)} geometry={adj.pass_geometry(1)}")
        t = measure({
            "istft": lambda: torch.autograd.grad(y_mf, X, gy, retain_graph=True),
            "composed": composed,
            "torch": lambda: torch.autograd.grad(y_th, X, gy, retain_graph=True),
            "stft": lambda: mf.fft(spec, gy3, plan=fwd),
        })
        row("istft bwd: the adjoint launch", t["istft"])
        row("(a) gy * inv_env, mf.stft, the c_k g / n product", t["composed"])
        row("(b) torch.autograd over torch.istft", t["torch"])
        row("(c) the plan_stft launch on the same bytes", t["stft"], fwd.kernel_name(1))
        ok = t["istft"][0] <= t["composed"][0] + (t["composed"][2] - t["composed"][1])
        met.append(ok)
        say(f"  istft bwd / (a) {ratio(t['istft'], t['composed'])}   istft bwd / (b) {ratio(t['istft'], t['torch'])}   "
            f"istft bwd / (c) {ratio(t['istft'], t['stft'])}   condition {'met' if ok else 'NOT met'}")
        del X, gy, y_mf, y_th, env, inv_env, got, ref, cmp, spec, gy3, adj, fwd
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        mf.clear_plan_cache()

    # ---- the MDCT pair: fp32, n = 256, the sine window; against torch.autograd over a dense cosine-matrix composition ----
    B, T, n, dt = 32, 480000, MDCT_N, torch.float32
    say(f"{B} x {T}, MDCT n {n}, float32")
    F = mf.mdct_frames(T, n)
    w = mf.mdct_window(n).to(DEV)
    j, k = torch.arange(2 * n, dtype=torch.float64, device=DEV)[None, :], torch.arange(n, dtype=torch.float64, device=DEV)[:, None]
    C = (torch.cos(math.pi / n * (j + 0.5 + n / 2.0) * (k + 0.5)) * w[None, :]).to(dt)  # (n, 2n), the window folded in

    def dense_mdct(x):
        xp = torch.nn.functional.pad(x, (n, (F + 1) * n - n - T))
        return xp.unfold(-1, 2 * n, n) @ C.T

    def dense_imdct(Z):
        y = (2.0 / n) * (Z @ C)
        out = torch.zeros(B, (F + 1) * n, dtype=dt, device=DEV)
        out[:, :F * n] = out[:, :F * n] + y[..., :n].reshape(B, F * n)
        out[:, n:] = out[:, n:] + y[..., n:].reshape(B, F * n)
        return out[:, n:n + T]

    x = torch.randn(B, T, dtype=dt, device=DEV).requires_grad_()
    Z = torch.randn(B, F, n, dtype=dt, device=DEV).requires_grad_()
    gX, gy = torch.randn(B, F, n, dtype=dt, device=DEV), torch.randn(B, T, dtype=dt, device=DEV)
    Xm, Xd = mf.mdct(x, n), dense_mdct(x)
    ym, yd = mf.imdct(Z, length=T), dense_imdct(Z)
    d1 = (torch.autograd.grad(Xm, x, gX, retain_graph=True)[0] - torch.autograd.grad(Xd, x, gX, retain_graph=True)[0]).abs().max()
    d2 = (torch.autograd.grad(ym, Z, gy, retain_graph=True)[0] - torch.autograd.grad(yd, Z, gy, retain_graph=True)[0]).abs().max()
    say(f"  against the dense composition: mdct bwd max abs difference {float(d1):.3e}, imdct bwd {float(d2):.3e}")
    t = measure({
        "mdct": lambda: torch.autograd.grad(Xm, x, gX, retain_graph=True),
        "mdct dense": lambda: torch.autograd.grad(Xd, x, gX, retain_graph=True),
        "imdct": lambda: torch.autograd.grad(ym, Z, gy, retain_graph=True),
        "imdct dense": lambda: torch.autograd.grad(yd, Z, gy, retain_graph=True),
    })
    row("mdct bwd: the plan_imdct launch", t["mdct"])
    row("torch.autograd over unfold @ C.T", t["mdct dense"])
    row("imdct bwd: the plan_mdct launch", t["imdct"])
    row("torch.autograd over Z @ C and two shifted adds", t["imdct dense"])
    say(f"  mdct bwd / dense {ratio(t['mdct'], t['mdct dense'])}   imdct bwd / dense {ratio(t['imdct'], t['imdct dense'])}   (report only)")
    say(f"condition (istft bwd not slower than (a) beyond the spread of (a)'s windows): "
        f"{'met at every shape' if all(met) else 'NOT met at ' + str(met.count(False)) + ' of ' + str(len(met)) + ' shapes'}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
