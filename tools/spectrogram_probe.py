"""Spectrogram plans (MIFFT_FLAG_STFT_POWER) beside the STFT plan they extend and the composition they replace, in one run per
shape (Hann window, centre reflect, power 2, an 80-band triangular mel filterbank generated here):
  (a) stft          mf.plan_stft + mf.fft: the complex spectrogram, the kernel the others are variants of;
  (b) power         mf.plan_spectrogram(power=2) + mf.fft: |X|^2 stored as reals (TileCfg::SPEC), half the stores of (a);
  (c) mel           the same with the filterbank (TileCfg::FB): 80 reals per frame;
  (d) composition   what (b) and (c) replace: mf.stft(...), .abs().pow(2), fb.T @ -- end to end, HIP events around the whole
                    sequence; (d') is the same without the filterbank product, the counterpart of (b);
  (e) torch         torch.stft(...).abs().pow(2) and fb.T @, where it runs.
Every figure is the MEDIAN of 7 windows of 20 calls, HIP events on the launch stream, after 5 warm-up calls; (a), (b) and (c) are
timed alternately, window by window, so that a drift of the machine hits all three, and their lowest and highest windows are
printed as the spread that a difference between them has to exceed.  Prints milliseconds, the bytes each variant has to move
at least (computed from the shapes), the kernel names, and the ratios (b)/(a), (b)/(d'), (c)/(d), (c)/(a).
    python tools/spectrogram_probe.py [out.txt]        (default: profiles/r11_spectrogram.txt)"""
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (batch, T, n_fft, hop, dtype): the shapes of tools/stft_probe.py
SHAPES = [(32, 480000, 400, 160, torch.float32),   # 30 s of 16-kHz speech, Whisper's front end
          (64, 220500, 1024, 256, torch.float32),
          (64, 220500, 2048, 512, torch.float32),
          (64, 220500, 1024, 256, torch.float64)]
BANDS = 80
WINDOWS, ITERS, WARMUP = 7, 20, 5


def mel_fb(n_fft, bands, rate=16000.0):
    """a triangular mel-style filterbank (n_fft // 2 + 1, bands) as float64 on the host: HTK mel scale, unnormalised"""
    K = n_fft // 2 + 1
    freqs = torch.linspace(0.0, rate / 2, K, dtype=torch.float64)
    mel = torch.linspace(0.0, 2595.0 * math.log10(1.0 + rate / 2 / 700.0), bands + 2, dtype=torch.float64)
    pts = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    up = (freqs[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None, :]
    down = (pts[None, 2:] - freqs[:, None]) / (pts[2:] - pts[1:-1])[None, :]
    return torch.clamp(torch.minimum(up, down), min=0.0)


def window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS


def timed(*fns):
    """(median, lowest, highest) milliseconds per call over the windows of every fn, their windows alternating"""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, fn in enumerate(fns):
            ms[k].append(window_ms(fn))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def report(label, t, nbytes, note):
    ms, lo, hi = t
    line = (f"  {label:<18} {ms:8.4f} ms [{lo:.4f} .. {hi:.4f}]  {nbytes / 1e6:9.1f} MB at least  "
            f"{nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s  {note}")
    print(line, flush=True)
    return line


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_spectrogram.txt")
    dev = "cuda:0"
    lines = [f"# tools/spectrogram_probe.py on {torch.cuda.get_device_name(0)}: median [lowest .. highest] of {WINDOWS} windows of "
             f"{ITERS} calls, HIP events on the launch stream, {WARMUP} warm-up calls; Hann window, centre reflect, power 2, "
             f"{BANDS} triangular mel bands",
             "# bytes: what the variant has to move at least, from the shapes -- (a) x + complex spectrogram; (b) x + real "
             "spectrogram; (c) x + bands; (d') (a), then the complex spectrogram read and the real one written; (d) (d'), then "
             "the real one read and the bands written"]
    for batch, T, n, hop, dtype in SHAPES:
        esz = 4 if dtype == torch.float32 else 8
        frames = mf.stft_frames(T, n, hop, True)
        h = n // 2 + 1
        fb64 = mel_fb(n, BANDS)
        spans = [int((fb64[:, m] != 0).sum()) for m in range(BANDS)]
        lines.append(f"{batch}x{T} n_fft={n} hop={hop} {'fp32' if dtype == torch.float32 else 'fp64'}: {frames} frames per signal; "
                     f"band spans {min(spans)} .. {max(spans)} bins, {sum(spans)} weights")
        print(lines[-1], flush=True)
        x = torch.randn(batch, T, device=dev, dtype=dtype)
        w = torch.hann_window(n, device=dev, dtype=dtype)
        fb = fb64.to(device=dev, dtype=dtype)
        x_b, cpx_b, real_b, mel_b = batch * T * esz, batch * frames * h * 2 * esz, batch * frames * h * esz, batch * frames * BANDS * esz
        x3 = x.reshape(batch, T, 1)
        ctx = mf.DeviceContext(0)

        plan_a = mf.plan_stft(dtype, batch, T, n, hop, window=w, center="reflect")
        plan_b = mf.plan_spectrogram(dtype, batch, T, n, hop, window=w, center="reflect", power=2)
        plan_c = mf.plan_spectrogram(dtype, batch, T, n, hop, window=w, center="reflect", power=2, fb=fb64)
        out_a = torch.empty(plan_a.out_shape, device=dev, dtype=dtype)
        out_b = torch.empty(plan_b.out_shape, device=dev, dtype=dtype)
        out_c = torch.empty(plan_c.out_shape, device=dev, dtype=dtype)

        def run_a():
            mf.fft(out_a, x3, ctx, plan=plan_a)

        def run_b():
            mf.fft(out_b, x3, ctx, plan=plan_b)

        def run_c():
            mf.fft(out_c, x3, ctx, plan=plan_c)

        def run_d1():
            return mf.stft(x, n, hop_length=hop, window=w).abs().pow(2)

        def run_d():
            return fb.T @ run_d1()

        # the routes agree before anything is timed
        run_a(), run_b(), run_c()
        ref_b, ref_c = run_d1().transpose(-1, -2), run_d().transpose(-1, -2)
        torch.cuda.synchronize()
        err_b = ((out_b[..., 0] - ref_b).norm() / ref_b.norm()).item()
        err_c = ((out_c[..., 0] - ref_c).norm() / ref_c.norm()).item()
        del ref_b, ref_c

        t_a, t_b, t_c = timed(run_a, run_b, run_c)
        t_d1, t_d = timed(run_d1, run_d)
        lines.append(report("(a) stft", t_a, x_b + cpx_b, f"{plan_a.kernel_name(1)} geometry {plan_a.pass_geometry(1)}"))
        lines.append(report("(b) power", t_b, x_b + real_b, f"{plan_b.kernel_name(1)} (agrees with (d') to {err_b:.1e})"))
        lines.append(report("(c) mel", t_c, x_b + mel_b, f"{plan_c.kernel_name(1)} (agrees with (d) to {err_c:.1e})"))
        lines.append(report("(d') stft, abs^2", t_d1, x_b + 2 * cpx_b + real_b, "mf.stft + .abs().pow(2)"))
        lines.append(report("(d) ... fb.T @", t_d, x_b + 2 * cpx_b + 2 * real_b + mel_b, "mf.stft + .abs().pow(2) + fb.T @"))
        ratios = (f"  ratios: (b)/(a) {t_b[0] / t_a[0]:.3f}   (b)/(d') {t_b[0] / t_d1[0]:.3f}   (b)/(d) {t_b[0] / t_d[0]:.3f}   "
                  f"(c)/(d) {t_c[0] / t_d[0]:.3f}   (c)/(a) {t_c[0] / t_a[0]:.3f}   (c)/(b) {t_c[0] / t_b[0]:.3f}")
        try:
            def run_e1():
                return torch.stft(x, n, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True).abs().pow(2)

            def run_e():
                return fb.T @ run_e1()

            got = run_e().transpose(-1, -2)
            err_e = ((got - out_c[..., 0]).norm() / got.norm()).item()
            del got
            t_e1, t_e = timed(run_e1, run_e)
            lines.append(report("(e') torch, abs^2", t_e1, x_b + 2 * cpx_b + real_b, "torch.stft + .abs().pow(2)"))
            lines.append(report("(e) ... fb.T @", t_e, x_b + 2 * cpx_b + 2 * real_b + mel_b, f"(agrees with (c) to {err_e:.1e})"))
            ratios += f"   (c)/(e) {t_c[0] / t_e[0]:.3f}"
        except Exception as e:  # (a build of torch without its FFT backend: said, not hidden)
            lines.append(f"  (e) torch            did not run: {type(e).__name__}: {str(e)[:120]}")
            print(lines[-1], flush=True)
        lines.append(ratios)
        print(ratios, flush=True)
        for p in (plan_a, plan_b, plan_c):
            p.close()
        mf.clear_plan_cache()
        del x, x3, out_a, out_b, out_c
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
