"""The log and post stages of a spectrogram plan (the tagged payload; TileCfg::LOG / TileCfg::POST) beside the mel plan they
extend and the torch kernels they replace, in one run per shape of tools/spectrogram_probe.py (Hann window, centre reflect,
power 2, its 80-band triangular mel filterbank):
  (c) mel          mf.plan_spectrogram(power=2, fb=) + mf.fft: the parent kernel, whose text the stages leave alone;
  (f) log-mel      the same with log="db": 10 log10(max(mel, 1e-10)) in the store;
  (g) mfcc         (f) with post=create_dct(13, 80): 13 reals per frame instead of 80;
  (d1) composition (c), then torch's clamp / log10 / scale over its output: what (f) replaces;
  (d2) composition (d1), then @ D: what (g) replaces.
Every figure is the MEDIAN of 7 windows of 20 calls, HIP events on the launch stream, after 5 warm-up calls; the five variants
are timed alternately, window by window, so that a drift of the machine hits all of them, and their lowest and highest windows
are printed as the spread that a difference between them has to exceed.  Prints milliseconds, the bytes each variant has to
move at least (from the shapes), the kernel names, and the ratios (f)/(c), (f)/(d1), (g)/(c), (g)/(d2).
    python tools/logmel_probe.py [out.txt]        (default: profiles/r12_logmel.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402
from spectrogram_probe import BANDS, ITERS, SHAPES, WARMUP, WINDOWS, mel_fb, report, timed  # noqa: E402

N_MFCC = 13
AMIN = 1e-10


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_logmel.txt")
    dev = "cuda:0"
    lines = [f"# tools/logmel_probe.py on {torch.cuda.get_device_name(0)}: median [lowest .. highest] of {WINDOWS} windows of "
             f"{ITERS} calls, HIP events on the launch stream, {WARMUP} warm-up calls, the variants in alternating windows; Hann "
             f"window, centre reflect, power 2, {BANDS} triangular mel bands, log=\"db\" (amin {AMIN:g}), a {BANDS} x {N_MFCC} "
             f"ortho DCT-II",
             "# bytes: what the variant has to move at least, from the shapes -- (c), (f) x + bands; (g) x + coefficients; (d1) "
             "(c), then the bands read and written; (d2) (d1), then the bands read and the coefficients written"]
    for batch, T, n, hop, dtype in SHAPES:
        esz = 4 if dtype == torch.float32 else 8
        frames = mf.stft_frames(T, n, hop, True)
        fb64 = mel_fb(n, BANDS)
        D64 = mf.create_dct(N_MFCC, BANDS)
        lines.append(f"{batch}x{T} n_fft={n} hop={hop} {'fp32' if dtype == torch.float32 else 'fp64'}: {frames} frames per signal")
        print(lines[-1], flush=True)
        x = torch.randn(batch, T, device=dev, dtype=dtype)
        w = torch.hann_window(n, device=dev, dtype=dtype)
        D = D64.to(device=dev, dtype=dtype)
        x_b, mel_b, cc_b = batch * T * esz, batch * frames * BANDS * esz, batch * frames * N_MFCC * esz
        x3 = x.reshape(batch, T, 1)
        ctx = mf.DeviceContext(0)
        kw = dict(window=w, center="reflect", power=2, fb=fb64)
        plan_c = mf.plan_spectrogram(dtype, batch, T, n, hop, **kw)
        plan_f = mf.plan_spectrogram(dtype, batch, T, n, hop, log="db", amin=AMIN, **kw)
        plan_g = mf.plan_spectrogram(dtype, batch, T, n, hop, log="db", amin=AMIN, post=D64, **kw)
        out_c = torch.empty(plan_c.out_shape, device=dev, dtype=dtype)
        out_f = torch.empty(plan_f.out_shape, device=dev, dtype=dtype)
        out_g = torch.empty(plan_g.out_shape, device=dev, dtype=dtype)
        assert plan_f.num_launches == plan_g.num_launches == 1 and plan_f.scratch_bytes == plan_g.scratch_bytes == 0

        def run_c():
            mf.fft(out_c, x3, ctx, plan=plan_c)

        def run_f():
            mf.fft(out_f, x3, ctx, plan=plan_f)

        def run_g():
            mf.fft(out_g, x3, ctx, plan=plan_g)

        def run_d1():
            run_c()
            return 10.0 * torch.log10(torch.clamp(out_c[..., 0], min=AMIN))

        def run_d2():
            return run_d1() @ D

        # the routes agree before anything is timed
        run_f(), run_g()
        ref_f, ref_g = run_d1(), run_d2()
        torch.cuda.synchronize()
        err_f = (out_f[..., 0] - ref_f).abs().max().item()
        err_g = ((out_g[..., 0] - ref_g).norm() / ref_g.norm()).item()
        del ref_f, ref_g

        t_c, t_f, t_g, t_d1, t_d2 = timed(run_c, run_f, run_g, run_d1, run_d2)
        lines.append(report("(c) mel", t_c, x_b + mel_b, f"{plan_c.kernel_name(1)} geometry {plan_c.pass_geometry(1)}"))
        lines.append(report("(f) log-mel", t_f, x_b + mel_b, f"{plan_f.kernel_name(1)} (within {err_f:.1e} dB of (d1))"))
        lines.append(report("(g) mfcc", t_g, x_b + cc_b, f"{plan_g.kernel_name(1)} (agrees with (d2) to {err_g:.1e})"))
        lines.append(report("(d1) (c), log10", t_d1, x_b + 3 * mel_b, "(c) + 10 * log10(clamp(.))"))
        lines.append(report("(d2) ... @ D", t_d2, x_b + 4 * mel_b + cc_b, "(c) + 10 * log10(clamp(.)) + @ D"))
        lines.append(f"  ratios: (f)/(c) {t_f[0] / t_c[0]:.3f}   (f)/(d1) {t_f[0] / t_d1[0]:.3f}   (g)/(c) {t_g[0] / t_c[0]:.3f}   "
                     f"(g)/(d2) {t_g[0] / t_d2[0]:.3f}   (g)/(f) {t_g[0] / t_f[0]:.3f}")
        print(lines[-1], flush=True)
        lines.append(f"  conditions: highest (f) {t_f[2]:.4f} < lowest (d1) {t_d1[1]:.4f}: {t_f[2] < t_d1[1]};   "
                     f"highest (g) {t_g[2]:.4f} < lowest (d2) {t_d2[1]:.4f}: {t_g[2] < t_d2[1]}")
        print(lines[-1], flush=True)
        for p in (plan_c, plan_f, plan_g):
            p.close()
        mf.clear_plan_cache()
        del x, x3, out_c, out_f, out_g
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
