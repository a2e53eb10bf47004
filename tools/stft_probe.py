"""STFT (MIFFT_FLAG_STFT) beside what the same spectrogram costs otherwise, in one run per shape (Hann window, centre
reflect):
  (a) stft          mf.plan_stft + mf.fft: the fused kernel (TileCfg::STFT), one launch, no padded copy, no tensor of frames;
  (b) composition   what it replaces: F.pad(reflect), unfold, window multiply made contiguous, mf.rfftn(onesided=True) -- end to
                    end, HIP events around the whole sequence;
  (c) rows alone    mf.rfftn's plan over the frames materialised beforehand: the floor -- the same stores with aligned,
                    non-overlapping loads;
  (d) torch.stft    where it runs.
Every figure is the MEDIAN of 7 windows of 20 calls, HIP events on the launch stream, after 5 warm-up calls; (a) and (c) are
timed alternately, window by window, so that a drift of the machine hits both.  Prints milliseconds, the bytes each variant has
to move at least (computed from the shapes), the kernel names, and the ratios (a)/(b), (a)/(c), (a)/(d).
    python tools/stft_probe.py [out.txt]        (default: profiles/r09_stft.txt)"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (batch, T, n_fft, hop, dtype)
SHAPES = [(32, 480000, 400, 160, torch.float32),   # 30 s of 16-kHz speech, Whisper's front end
          (64, 220500, 1024, 256, torch.float32),
          (64, 220500, 2048, 512, torch.float32),
          (64, 220500, 1024, 256, torch.float64)]
WINDOWS, ITERS, WARMUP = 7, 20, 5


def window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS


def timed(*fns):
    """median milliseconds per call of every fn, their windows alternating"""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, fn in enumerate(fns):
            ms[k].append(window_ms(fn))
    return [statistics.median(m) for m in ms]


def report(label, ms, nbytes, note):
    line = f"  {label:<18} {ms:8.4f} ms  {nbytes / 1e6:9.1f} MB at least  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s  {note}"
    print(line, flush=True)
    return line


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_stft.txt")
    dev = "cuda:0"
    lines = [f"# tools/stft_probe.py on {torch.cuda.get_device_name(0)}: median of {WINDOWS} windows of {ITERS} calls, HIP events on "
             f"the launch stream, {WARMUP} warm-up calls; Hann window, centre reflect",
             "# bytes: what the variant has to move at least, from the shapes -- (a) x + spectrogram; (b) pad copy (x read and "
             "written), frames written and read (unfold * window, then the transform), spectrogram; (c) frames + spectrogram"]
    for batch, T, n, hop, dtype in SHAPES:
        esz = 4 if dtype == torch.float32 else 8
        frames = mf.stft_frames(T, n, hop, True)
        h = n // 2 + 1
        lines.append(f"{batch}x{T} n_fft={n} hop={hop} {'fp32' if dtype == torch.float32 else 'fp64'}: {frames} frames per signal")
        print(lines[-1], flush=True)
        x = torch.randn(batch, T, device=dev, dtype=dtype)
        w = torch.hann_window(n, device=dev, dtype=dtype)
        spec_b, x_b, fr_b = batch * frames * h * 2 * esz, batch * T * esz, batch * frames * n * esz

        plan = mf.plan_stft(dtype, batch, T, n, hop, window=w, center="reflect")
        out = torch.empty(plan.out_shape, device=dev, dtype=dtype)
        x3 = x.reshape(batch, T, 1)
        ctx = mf.DeviceContext(0)

        def run_a():
            mf.fft(out, x3, ctx, plan=plan)

        def materialise():
            xp = F.pad(x.unsqueeze(1), (n // 2, n // 2), mode="reflect").squeeze(1)
            return (xp.unfold(-1, n, hop) * w).contiguous()

        def run_b():
            return mf.rfftn(materialise().reshape(batch * frames, n), onesided=True)

        fr = materialise().reshape(batch * frames, n, 1)
        rows = mf.plan_fft(dtype, dtype, fr.shape, (batch * frames, h, 2), half_spectrum=True)
        out_c = torch.empty((batch * frames, h, 2), device=dev, dtype=dtype)

        def run_c():
            mf.fft(out_c, fr, ctx, plan=rows)

        # the three routes agree before anything is timed
        run_a()
        ref = torch.view_as_real(run_b()).reshape(out.shape)
        run_c()
        torch.cuda.synchronize()
        err_b = ((out - ref).norm() / ref.norm()).item()
        err_c = ((out - out_c.reshape(out.shape)).norm() / ref.norm()).item()

        t_a, t_c = timed(run_a, run_c)
        (t_b,) = timed(run_b)
        lines.append(report("(a) stft", t_a, x_b + spec_b, f"{plan.kernel_name(1)} geometry {plan.pass_geometry(1)}"))
        lines.append(report("(b) composition", t_b, 2 * (x_b + batch * n * esz) + 2 * fr_b + spec_b,
                            f"pad + unfold * window + rfftn(onesided) (agrees with (a) to {err_b:.1e})"))
        lines.append(report("(c) rows alone", t_c, fr_b + spec_b,
                            f"{rows.kernel_name(0)} geometry {rows.pass_geometry(0)} (agrees with (a) to {err_c:.1e})"))
        ratios = f"  ratios: (a)/(b) {t_a / t_b:.3f}   (a)/(c) {t_a / t_c:.3f}"
        del fr, out_c, ref
        try:
            def run_d():
                return torch.stft(x, n, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)

            got = run_d().transpose(-1, -2)
            err_d = ((torch.view_as_real(got) - out).norm() / out.norm()).item()
            (t_d,) = timed(run_d)
            lines.append(report("(d) torch.stft", t_d, x_b + spec_b, f"(agrees with (a) to {err_d:.1e})"))
            ratios += f"   (a)/(d) {t_a / t_d:.3f}"
        except Exception as e:  # (a build of torch without its FFT backend: said, not hidden)
            lines.append(f"  (d) torch.stft       did not run: {type(e).__name__}: {str(e)[:120]}")
            print(lines[-1], flush=True)
        lines.append(ratios)
        print(ratios, flush=True)
        plan.close()
        rows.close()
        del x, out, x3
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
