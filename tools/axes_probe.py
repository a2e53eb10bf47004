"""Transforms over a subset of the dims (MIFFT_FLAG_KEEP_DIM): each masked shape timed with time_fft beside the 100000 x 1024
C2C rows (the same bytes as the first three shapes) and, alternating in the same process, beside the same plan with the
interleaved block tile switched off (MIFFT_ILV=0: the column tiles).  MIFFT_ILV is a lab-build switch, re-read per plan:
run with MIFFT_LIBRARY pointing at libmifft_lab.so (the product library ignores it and both columns show the tile).
Prints, per shape: milliseconds (best of 3 x 20 execs), HBM bytes of x + out, their rate as a fraction of 8 TB/s and the
kernel names of the transformed dims.
    MIFFT_LIBRARY=hackathon_fft_amd/csrc/libmifft_lab.so python tools/axes_probe.py [out.txt]
                                                                   (default: profiles/r05_axes.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

# (logical shape, torch dim)
SHAPES = [((50000, 1024, 2), (1,)), ((25000, 1024, 4), (1,)), ((12500, 1024, 8), (1,)), ((100, 480, 640, 3), (1, 2)),
          ((1000, 1024, 100), (1,))]
ROWS = (100000, 1024)
PEAK = 8.0e12  # bytes / s


def make_plan(layout, axes, ilv):
    os.environ["MIFFT_ILV"] = "1" if ilv else "0"
    try:
        return mf.plan_fft(torch.float32, torch.float32, layout, layout, axes=axes)
    finally:
        os.environ.pop("MIFFT_ILV", None)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r05_axes.txt")
    lib = os.path.basename(mf.LIB_PATH)
    lines = [f"# tools/axes_probe.py on {torch.cuda.get_device_name(0)} ({lib}), fp32, best of 3 x 20 execs (time_fft),",
             "# the three variants of a shape alternating within each of the 3 rounds",
             "# bytes = x + out, each moved once; fraction of 8 TB/s = bytes / time / 8e12"]
    for ln in lines:
        print(ln, flush=True)
    dev = "cuda:0"
    ctx = mf.DeviceContext(0)
    rx = torch.randn(ROWS + (2,), device=dev)
    rout = torch.empty_like(rx)
    rplan = mf.plan_fft(torch.float32, torch.float32, rx.shape, rout.shape)
    for shape, dim in SHAPES:
        layout, axes = mf.reduce_dims(shape, dim)
        layout = layout + (2,)
        x = torch.randn(layout, device=dev)
        out = torch.empty_like(x)
        variants = [("interleaved tile", make_plan(layout, axes, True), x, out),
                    ("MIFFT_ILV=0 (columns)", make_plan(layout, axes, False), x, out),
                    (f"C2C rows {ROWS[0]}x{ROWS[1]}", rplan, rx, rout)]
        best = [float("inf")] * len(variants)
        for _, p, a, b in variants:
            mf.time_fft(b, a, plan=p, iters=5, ctx=ctx)
        for _ in range(3):
            for k, (_, p, a, b) in enumerate(variants):
                best[k] = min(best[k], mf.time_fft(b, a, plan=p, iters=20, ctx=ctx))
        lines.append(f"{'x'.join(map(str, shape))} dim={dim}:")
        print(lines[-1], flush=True)
        for k, (label, p, a, b) in enumerate(variants):
            nbytes = a.numel() * a.element_size() + b.numel() * b.element_size()
            names = " / ".join(p.kernel_name(d) for d in range(p.ndim) if p.kernel_name(d) != "none")
            frac = nbytes / (best[k] * 1e-3) / PEAK
            lines.append(f"  {label:<24} {best[k]:8.4f} ms  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {names}")
            print(lines[-1], flush=True)
        lines.append(f"  interleaved / columns {best[0] / best[1]:.3f}, interleaved / rows {best[0] / best[2]:.3f}")
        print(lines[-1], flush=True)
        del variants, x, out
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
