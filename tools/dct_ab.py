"""A/B of the DCT kernels' LDS-side permutation (TileCfg::DCT_QUADS): four reals per thread (the product's code) against pairs
(-DMIFFT_DCT_PAIRS), each variant runtime-specialised by the lab library in a fresh child process with its own kernel cache,
beside the half-spectrum R2C / C2R kernels of the same rows.  fp32, best of 3 x 20 execs (time_fft), ms.
    python tools/dct_ab.py [out.txt]        (default: profiles/r06_dct_ab.txt; needs hackathon_fft_amd/csrc/libmifft_lab.so)"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(500000, 128), (102400, 1000), (50000, 2048), (200000, 480), (12500, 8192)]  # (no precompiled DCT instance)
VARIANTS = [("quads (product)", ""), ("pairs", "-DMIFFT_DCT_PAIRS=1")]


def child():
    import torch
    sys.path.insert(0, ROOT)
    import hackathon_fft_amd as mf

    def timed(plan, out, x):
        with mf.DeviceContext(0) as ctx:
            mf.time_fft(out, x, plan=plan, iters=5, ctx=ctx)
            return min(mf.time_fft(out, x, plan=plan, iters=20, ctx=ctx) for _ in range(3))

    f32 = torch.float32
    for b, n in SHAPES:
        x = torch.randn(b, n, 1, device="cuda:0")
        o = torch.empty_like(x)
        h = torch.empty(b, n // 2 + 1, 2, device="cuda:0")
        t, names = [], []
        for inv in (False, True):
            p = mf.plan_fft(f32, f32, x.shape, o.shape, inverse=inv, dct=True)
            t.append(timed(p, o, x))
            names.append(p.kernel_name(0))
        p = mf.plan_fft(f32, f32, x.shape, h.shape, half_spectrum=True)
        t.append(timed(p, h, x))
        p = mf.plan_fft(f32, f32, h.shape, o.shape, inverse=True, half_spectrum=True)
        t.append(timed(p, o, h))
        print(f"  {b}x{n}: dct {t[0]:.4f}  idct {t[1]:.4f}  r2c {t[2]:.4f}  c2r {t[3]:.4f}  {names[0]} {names[1]}", flush=True)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_dct_ab.txt")
    lab = os.path.join(ROOT, "hackathon_fft_amd", "csrc", "libmifft_lab.so")
    lines = ["# tools/dct_ab.py: DCT kernels with four reals per thread in the LDS-side permutation against pairs, fp32,",
             "# best of 3 x 20 execs (time_fft), ms; r2c / c2r: the half-spectrum kernels of the same rows"]
    for label, defines in VARIANTS:
        with tempfile.TemporaryDirectory() as cache:
            env = dict(os.environ, MIFFT_LIBRARY=lab, MIFFT_JIT_DEFINES=defines, MIFFT_JIT_CACHE_DIR=cache, MIFFT_DCT_AB_CHILD="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"{label}: child failed ({r.returncode})\n{r.stderr[-2000:]}")
        lines.append(f"{label}  MIFFT_JIT_DEFINES={defines!r}:")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("  ")]
        print("\n".join(lines[-len(SHAPES) - 1:]), flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    child() if os.environ.get("MIFFT_DCT_AB_CHILD") else main()
