"""Half-spectrum real transforms (MIFFT_FLAG_HALF_SPECTRUM): forward (R2C rows + columns over n // 2 + 1 bins) and inverse
(columns + C2R rows) timed with time_fft, each beside the full-spectrum real plan and the complex plan of the same shape.
Prints, per shape: milliseconds (best of 3 x 20 execs), HBM bytes of the tensors read and written once (x + out; the inverse
scratch passes are not counted), their rate as a fraction of 8 TB/s, and the kernel names.
    python tools/half_spectrum_probe.py [out.txt]        (default: profiles/r04_half_spectrum.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

SHAPES = [(100000, 1024), (250000, 128), (100, 640, 480), (10, 1920, 1080), (100, 64, 64, 64), (10, 128, 128, 128)]
PEAK = 8.0e12  # bytes / s


def timed(plan, out, x):
    with mf.DeviceContext(0) as ctx:
        mf.time_fft(out, x, plan=plan, iters=5, ctx=ctx)
        return min(mf.time_fft(out, x, plan=plan, iters=20, ctx=ctx) for _ in range(3))


def row(label, plan, x, out):
    ms = timed(plan, out, x)
    nbytes = x.numel() * x.element_size() + out.numel() * out.element_size()
    names = " / ".join(plan.kernel_name(d) for d in range(plan.ndim))
    frac = nbytes / (ms * 1e-3) / PEAK
    line = f"  {label:<22} {ms:8.4f} ms  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {names}"
    print(line, flush=True)
    return line


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r04_half_spectrum.txt")
    lines = [f"# tools/half_spectrum_probe.py on {torch.cuda.get_device_name(0)}, fp32, best of 3 x 20 execs (time_fft)",
             "# bytes = x + out, each moved once; fraction of 8 TB/s = bytes / time / 8e12"]
    dev = "cuda:0"
    for shape in SHAPES:
        n = shape[-1]
        h = n // 2 + 1
        lines.append(f"{'x'.join(map(str, shape))}:")
        print(lines[-1], flush=True)
        real = torch.randn(shape + (1,), device=dev)
        half = torch.empty(shape[:-1] + (h, 2), device=dev)
        p = mf.plan_fft(torch.float32, torch.float32, real.shape, half.shape, half_spectrum=True)
        lines.append(row("forward half (R2C)", p, real, half))
        del p
        back = torch.empty(shape + (1,), device=dev)
        p = mf.plan_fft(torch.float32, torch.float32, half.shape, back.shape, inverse=True, half_spectrum=True)
        lines.append(row("inverse half (C2R)", p, half, back))
        del p, back
        full = torch.empty(shape + (2,), device=dev)
        p = mf.plan_fft(torch.float32, torch.float32, real.shape, full.shape)
        lines.append(row("full-spectrum real", p, real, full))
        del p, real
        cx = torch.randn(shape + (2,), device=dev)
        p = mf.plan_fft(torch.float32, torch.float32, cx.shape, full.shape)
        lines.append(row("C2C forward", p, cx, full))
        del p, cx, full, half
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
