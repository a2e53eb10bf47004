"""N-D DCT (MIFFT_FLAG_DCT_ND) beside what the same tensor cost before and beside the passes it is made of, per shape:
  (a) dctn / idctn       mf.dctn over the two / three inner dims: the packed-row DCT kernel + one paired-column pass per other dim;
  (b) composition        what it replaces, in the same process: mf.dct -> transpose(-1, -2).contiguous() -> mf.dct -> transpose
                         back (.contiguous()), 2-D shapes; HIP events around the whole sequence;
  (c) complex columns    mf.fftn(dim=1) of the (B, H, W / 2) complex view: the in-place column pass over the same bytes through
                         the same butterflies, without the DCT's permutation and combine (out of place here: + one read of x);
  (d) rows alone         the packed-row DCT pass (a plan with every other dim kept), and the column pass alone.
Also the A/B of the forward column tile's load: rows permuted in the direct pass-0 load against a staging copy through LDS
(MIFFT_DCT_COLS_DIRECT, a lab-build switch re-read per plan: run with MIFFT_LIBRARY pointing at libmifft_lab.so; the product
library ignores it and both lines show the same kernel).
Read-only timing loops (best of 3 x 20 execs).  Every shape is a step in a child process with its own time limit; the first
step that fails or runs out of time ends the run.
    python tools/dctn_probe.py [out.txt]        (default: profiles/r08_dctn.txt)"""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

STEPS = [((100, 640, 480), "fp32"), ((10, 128, 128, 128), "fp32"), ((100, 640, 480), "fp64")]
STEP_LIMIT = 150  # seconds per step
PEAK = 8.0e12     # bytes / s
DT = {"fp32": torch.float32, "fp64": torch.float64}


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
    print(f"  {label:<34} {ms:8.4f} ms  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {names}", flush=True)


def names_of(plan):
    return " + ".join(plan.kernel_name(d) for d in reversed(range(plan.ndim)) if plan.kernel_name(d) != "none")


def composed(x, inverse):
    f = mf.idct if inverse else mf.dct
    return f(f(x).transpose(-1, -2).contiguous()).transpose(-1, -2).contiguous()


def step(shape, tag):
    dtype = DT[tag]
    esz = 4 if dtype == torch.float32 else 8
    dev = "cuda:0"
    nd = len(shape) - 1
    print(f"{'x'.join(str(v) for v in shape)} {tag}:", flush=True)
    x = torch.randn(shape + (1,), device=dev, dtype=dtype)
    out = torch.empty_like(x)
    numel = x.numel()
    once = 2 * numel * esz  # x read once, out written once
    t = {}
    for inverse, nm in ((False, "dctn"), (True, "idctn")):
        p = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dctn=True)
        t[nm] = timed(p, out, x)
        report(f"(a) {nm}", t[nm], once * nd, names_of(p))  # (every pass moves the tensor once each way)
        # (d) the passes alone: the rows x -> out, the columns over dim 1 x -> out
        p = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dctn=True, axes=(nd,))
        t[nm + " rows"] = timed(p, out, x)
        report(f"(d) {nm} rows alone", t[nm + " rows"], once, names_of(p))
        for direct in ((True, False) if not inverse else (True,)):
            os.environ["MIFFT_DCT_COLS_DIRECT"] = "1" if direct else "0"
            p = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dctn=True, axes=(1,))
            os.environ.pop("MIFFT_DCT_COLS_DIRECT", None)
            key = nm + " cols" + ("" if direct else " staged")
            t[key] = timed(p, out, x)
            label = f"(d) {nm} columns alone (dim 1)" if inverse else f"(d) {nm} columns, {'direct' if direct else 'staged'} load"
            report(label, t[key], once, names_of(p))
    # (c) the complex column pass over the same bytes
    xc = torch.view_as_complex(x.reshape(shape[:-1] + (shape[-1] // 2, 2)))
    for inverse, nm, f in ((False, "fftn", mf.fftn), (True, "ifftn", mf.ifftn)):
        t[nm] = timed_fn(lambda: f(xc, dim=1))
        report(f"(c) complex columns, {nm}(dim=1)", t[nm], once, "out of place: as the columns alone of (d)")
    if nd == 2:  # (b) the composition it replaces
        x2 = x.squeeze(-1)
        ref = mf.dctn(x2[:2])
        err = ((composed(x2[:2], False) - ref).norm() / ref.norm()).item()
        for inverse, nm in ((False, "dctn"), (True, "idctn")):
            t["comp " + nm] = timed_fn(lambda: composed(x2, inverse))
            report(f"(b) composition of {nm}", t["comp " + nm], once * 4, f"dct + transpose + dct + transpose (agrees to {err:.1e})")
        print(f"  ratios: composition / dctn {t['comp dctn'] / t['dctn']:.2f}   composition / idctn "
              f"{t['comp idctn'] / t['idctn']:.2f}", flush=True)
    print(f"  ratios: dct columns / complex columns {t['dctn cols'] / t['fftn']:.3f}   idct columns / complex columns "
          f"{t['idctn cols'] / t['ifftn']:.3f}   staged / direct load {t['dctn cols staged'] / t['dctn cols']:.3f}", flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        i = int(sys.argv[2])
        step(*STEPS[i])
        return 0
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_dctn.txt")
    lines = [f"# tools/dctn_probe.py on {torch.cuda.get_device_name(0)}, best of 3 x 20 execs (time_fft; wrappers: HIP events "
             f"around the whole sequence)",
             "# bytes = the tensor read once and written once per pass; fraction of 8 TB/s = bytes / time / 8e12",
             f"# library: {os.environ.get('MIFFT_LIBRARY', 'libmifft.so (MIFFT_DCT_COLS_DIRECT ignored: staged = direct)')}"]
    rc = 0
    for i in range(len(STEPS)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(i)], capture_output=True, text=True,
                               timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"step {i} {STEPS[i]}: no result within {STEP_LIMIT} s; stopped")
            rc = 1
            break
        lines.append(r.stdout.rstrip())
        print(r.stdout, flush=True)
        if r.returncode != 0:
            lines.append(f"step {i} {STEPS[i]} failed (exit status {r.returncode}); stopped\n{r.stderr[-2000:]}")
            print(lines[-1], flush=True)
            rc = 1
            break
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")
    return rc


if __name__ == "__main__":
    sys.exit(main())
