"""Inverse STFT (MIFFT_FLAG_ISTFT) beside what the same signal costs otherwise, in one run per shape (Hann window, centred):
  (a) istft         mf.plan_istft + mf.fft: the fused kernel (TileCfg::ISTFT), one launch, no tensor of frames, no memset --
                    once per value of istft_min_run (1, 2, 4, 8, 16) when the loaded library is the lab build
                    (MIFFT_LIBRARY=hackathon_fft_amd/csrc/libmifft_lab.so, knob MIFFT_ISTFT_MIN_RUN), else at the default;
  (b) composition   what it replaces: mf.irfftn of the frames, window multiply, torch.nn.functional.fold, divide by the
                    envelope, trim -- end to end, HIP events around the whole sequence;
  (c) torch.istft   on the device, where it runs;
  (d) rows alone    the plain C2R rows of the same frames (mf.irfftn's plan): the floor of the transform, without overlap-add;
  (e) copy          a device copy that reads and writes as many bytes as (a) has to move at least.
Every figure is the MEDIAN of 7 windows of 20 calls, HIP events on the launch stream, after 5 warm-up calls, with the spread
(min .. max of the windows); the variants of (a) and (d) are timed alternately, window by window, so that a drift of the machine
hits all of them.  Prints milliseconds, the bytes each variant has to move at least (from the shapes), kernel names, geometry.
    python tools/istft_probe.py [out.txt]        (default: profiles/r10_istft.txt)"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402
from hackathon_fft_amd import _lib  # noqa: E402

# (batch, samples, n_fft, hop, dtype)
SHAPES = [(32, 480000, 400, 160, torch.float32),   # 30 s of 16-kHz speech
          (32, 220500, 1024, 256, torch.float32),  # 5 s of 44.1-kHz audio
          (2, 480000, 400, 160, torch.float32),    # a few hundred tiles: where istft_min_run decides the grid
          (3, 220500, 1024, 256, torch.float32)]
MIN_RUNS = (1, 2, 4, 8, 16)
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
    """(median, min, max) milliseconds per call of every fn, their windows alternating"""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, fn in enumerate(fns):
            ms[k].append(window_ms(fn))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_istft.txt")
    dev = "cuda:0"
    lab = "lab" in os.path.basename(_lib.LIB_PATH)
    lines = [f"# tools/istft_probe.py on {torch.cuda.get_device_name(0)}: median (min .. max) of {WINDOWS} windows of {ITERS} calls, "
             f"HIP events on the launch stream, {WARMUP} warm-up calls; Hann window, centred; library {os.path.basename(_lib.LIB_PATH)}",
             "# bytes: what the variant has to move at least, from the shapes -- (a) spectrogram + signal; (b) spectrogram, frames "
             "written (irfftn), read and written (window), read (fold), padded signal written, read and written (divide, trim); "
             "(d) spectrogram + frames; (e) as (a)"]

    def report(label, t, nbytes, note):
        ms, lo, hi = t
        line = (f"  {label:<22} {ms:8.4f} ms ({lo:.4f} .. {hi:.4f})  {nbytes / 1e6:8.1f} MB at least  "
                f"{nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s  {note}")
        print(line, flush=True)
        lines.append(line)

    for batch, T, n, hop, dtype in SHAPES:
        esz = 4 if dtype == torch.float32 else 8
        frames = mf.stft_frames(T, n, hop, True)
        h, L = n // 2 + 1, n + hop * (frames - 1)
        lines.append(f"{batch}x{T} n_fft={n} hop={hop} {'fp32' if dtype == torch.float32 else 'fp64'}: {frames} frames per signal")
        print(lines[-1], flush=True)
        ctype = torch.complex64 if dtype == torch.float32 else torch.complex128
        X = torch.randn(batch, frames, h, device=dev, dtype=ctype)   # frames-major, as the kernel reads it
        Xr = torch.view_as_real(X)
        w = torch.hann_window(n, device=dev, dtype=dtype)
        spec_b, sig_b, fr_b, pad_b = batch * frames * h * 2 * esz, batch * T * esz, batch * frames * n * esz, batch * L * esz
        ctx = mf.DeviceContext(0)
        out = torch.empty((batch, T, 1), device=dev, dtype=dtype)

        plans = []
        for mr in (MIN_RUNS if lab else (None,)):
            if mr is not None:
                os.environ["MIFFT_ISTFT_MIN_RUN"] = str(mr)
            plans.append((mr, mf.plan_istft(dtype, batch, frames, n, hop, window=w, center=True, length=T)))
        os.environ.pop("MIFFT_ISTFT_MIN_RUN", None)

        env = F.fold((w * w).reshape(1, n, 1).expand(1, n, frames), (1, L), (1, n), stride=(1, hop)).reshape(L)[n // 2:n // 2 + T]

        def run_b():
            y = mf.irfftn(X.reshape(batch * frames, h), n).reshape(batch, frames, n) * w
            s = F.fold(y.transpose(1, 2), (1, L), (1, n), stride=(1, hop)).reshape(batch, L)
            return s[:, n // 2:n // 2 + T] / env

        rows = mf.plan_fft(dtype, dtype, (batch * frames, h, 2), (batch * frames, n, 1), half_spectrum=True, inverse=True)
        out_d = torch.empty((batch * frames, n, 1), device=dev, dtype=dtype)
        Xrows = Xr.reshape(batch * frames, h, 2)

        def run_d():
            mf.fft(out_d, Xrows, ctx, plan=rows)

        half = (spec_b + sig_b) // 2 // esz
        src, dst = torch.randn(half, device=dev, dtype=dtype), torch.empty(half, device=dev, dtype=dtype)

        def run_e():
            dst.copy_(src)

        # the routes agree before anything is timed
        ref = run_b()
        torch.cuda.synchronize()
        runs_a = []
        for mr, plan in plans:
            out.fill_(float("nan"))
            mf.fft(out, Xr, ctx, plan=plan)
            torch.cuda.synchronize()
            err = ((out.reshape(batch, T) - ref).norm() / ref.norm()).item()
            runs_a.append((mr, plan, err, (lambda p: (lambda: mf.fft(out, Xr, ctx, plan=p)))(plan)))
        del ref

        ts = timed(*[r[3] for r in runs_a], run_d, run_e)
        for (mr, plan, err, _), t in zip(runs_a, ts):
            sched = mf.istft_schedule(plan)
            warm = sum(r[2] for r in sched)
            report(f"(a) istft min_run={mr if mr is not None else 'default'}", t, spec_b + sig_b,
                   f"{plan.kernel_name(2)} geometry {plan.pass_geometry(2)} warm-up tiles {warm} (agrees with (b) to {err:.1e})")
        (t_b,) = timed(run_b)
        report("(b) composition", t_b, spec_b + 4 * fr_b + 3 * pad_b + sig_b, "irfftn + window + fold + divide")
        try:
            def run_c():
                return torch.istft(X.transpose(-1, -2), n, hop_length=hop, window=w, center=True, length=T)

            run_c()
            (t_c,) = timed(run_c)
            report("(c) torch.istft", t_c, spec_b + sig_b, "")
        except Exception as e:  # (a build of torch without its FFT backend: said, not hidden)
            lines.append(f"  (c) torch.istft        did not run: {type(e).__name__}: {str(e)[:120]}")
            print(lines[-1], flush=True)
            t_c = None
        report("(d) rows alone", ts[-2], spec_b + fr_b, f"{rows.kernel_name(0)} geometry {rows.pass_geometry(0)}")
        report("(e) copy", ts[-1], spec_b + sig_b, "torch copy_ of half these bytes")
        best = min(zip(ts, runs_a), key=lambda z: z[0][0])
        ratios = (f"  ratios of the fastest (a) (min_run={best[1][0]}): /(b) {best[0][0] / t_b[0]:.3f}   /(d) {best[0][0] / ts[-2][0]:.3f}   "
                  f"/(e) {best[0][0] / ts[-1][0]:.3f}" + (f"   /(c) {best[0][0] / t_c[0]:.3f}" if t_c else ""))
        lines.append(ratios)
        print(ratios, flush=True)
        for _, plan in plans:
            plan.close()
        rows.close()
        del X, Xr, Xrows, out, out_d, src, dst
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
