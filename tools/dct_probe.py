"""DCT-II / inverse (MIFFT_FLAG_DCT) beside what the same rows cost otherwise, in one run per shape:
  dct / idct               the fused packed-row kernels (TileCfg::DCT), one launch each;
  R2C / C2R                the half-spectrum forward and inverse of the same rows (kernels this feature does not touch);
  composition              what a DCT-II took before: torch index permutation, mf.rfftn(onesided=True), torch twiddle multiply
                           taking .real -- timed with HIP events around the whole sequence.
Prints milliseconds (best of 3 x 20 execs), the HBM bytes of x + out moved once, their rate as a fraction of 8 TB/s, the
kernel names and the ratios dct / R2C, idct / C2R and composition / dct.
    python tools/dct_probe.py [out.txt]        (default: profiles/r06_dct.txt)"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

SHAPES = [((100000, 1024), torch.float32), ((500000, 128), torch.float32), ((100000, 1024), torch.float64)]
PEAK = 8.0e12  # bytes / s


def timed(plan, out, x):
    with mf.DeviceContext(0) as ctx:
        mf.time_fft(out, x, plan=plan, iters=5, ctx=ctx)
        return min(mf.time_fft(out, x, plan=plan, iters=20, ctx=ctx) for _ in range(3))


def timed_fn(fn, iters=20):
    for _ in range(5):
        fn()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters)
    return best


def report(label, ms, nbytes, names):
    frac = nbytes / (ms * 1e-3) / PEAK
    line = f"  {label:<22} {ms:8.4f} ms  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {names}"
    print(line, flush=True)
    return line


def composed_dct(x, perm, tw):
    """DCT-II from the pieces available without MIFFT_FLAG_DCT (Makhoul): gather, one-sided real FFT, twiddle, mirror"""
    n = x.shape[-1]
    V = mf.rfftn(x[:, perm], onesided=True)  # (batch, n // 2 + 1)
    t = V * tw
    return torch.cat([2 * t.real, (-2 * t.imag[:, 1:n // 2]).flip(-1)], dim=-1)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_dct.txt")
    lines = [f"# tools/dct_probe.py on {torch.cuda.get_device_name(0)}, best of 3 x 20 execs (time_fft; the composition: HIP "
             f"events around the whole sequence)",
             "# bytes = x + out, each moved once; fraction of 8 TB/s = bytes / time / 8e12"]
    dev = "cuda:0"
    for shape, dtype in SHAPES:
        batch, n = shape
        h = n // 2 + 1
        esz = 4 if dtype == torch.float32 else 8
        lines.append(f"{batch}x{n} {'fp32' if dtype == torch.float32 else 'fp64'}:")
        print(lines[-1], flush=True)
        real = torch.randn(shape + (1,), device=dev, dtype=dtype)
        out = torch.empty(shape + (1,), device=dev, dtype=dtype)
        rr = 2 * batch * n * esz
        p = mf.plan_fft(dtype, dtype, real.shape, out.shape, dct=True)
        t_dct = timed(p, out, real)
        lines.append(report("dct", t_dct, rr, p.kernel_name(0)))
        p = mf.plan_fft(dtype, dtype, real.shape, out.shape, inverse=True, dct=True)
        t_idct = timed(p, out, real)
        lines.append(report("idct", t_idct, rr, p.kernel_name(0)))
        half = torch.empty((batch, h, 2), device=dev, dtype=dtype)
        rh = batch * (n + 2 * h) * esz
        p = mf.plan_fft(dtype, dtype, real.shape, half.shape, half_spectrum=True)
        t_r2c = timed(p, half, real)
        lines.append(report("forward half (R2C)", t_r2c, rh, p.kernel_name(0)))
        p = mf.plan_fft(dtype, dtype, half.shape, out.shape, inverse=True, half_spectrum=True)
        t_c2r = timed(p, out, half)
        lines.append(report("inverse half (C2R)", t_c2r, rh, p.kernel_name(0)))
        del p, half, out
        x2 = real.squeeze(-1)
        perm = torch.cat([torch.arange(0, n, 2), torch.arange(n - 1, 0, -2)]).to(dev)
        k = torch.arange(h, device=dev, dtype=torch.float64)
        tw = torch.polar(torch.ones_like(k), -math.pi * k / (2 * n)).to(torch.complex64 if dtype == torch.float32
                                                                          else torch.complex128)
        ref = mf.dct(x2[:64])
        err = ((composed_dct(x2[:64], perm, tw) - ref).norm() / ref.norm()).item()
        t_comp = timed_fn(lambda: composed_dct(x2, perm, tw))
        lines.append(report("composition", t_comp, rr, f"gather + rfftn(onesided) + twiddle (agrees with dct to {err:.1e})"))
        lines.append(f"  ratios: dct / R2C {t_dct / t_r2c:.3f}   idct / C2R {t_idct / t_c2r:.3f}   "
                     f"composition / dct {t_comp / t_dct:.2f}")
        print(lines[-1], flush=True)
        del real, x2
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
