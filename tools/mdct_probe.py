"""DCT-IV rows (MIFFT_DCT_TYPE4_TAG) and the fused MDCT (MIFFT_MDCT_TAG) beside their yardsticks, in one process per run:
  (a) dct(type=4) rows against dct(type=2) rows of the same shape (equal bytes: type 2 is the yardstick) and against the
      composition it replaces: torch gather + twiddle + mf.fftn of n / 2 complex points + twiddle + scatter;
  (b) plan_mdct against its composition -- F.pad + unfold + window + fold with torch + dct(type=4) -- and against the floor:
      the DCT-IV rows over folded frames materialised beforehand (the fold's traffic not counted).
Timing: HIP events around windows of 20 calls, the variants of a shape alternating window by window inside the process, 5
warm-up calls each first; the figure is the median of 7 windows, the spread their min .. max.  Bytes are the fused kernel's
own traffic (x once + out once); the rate is given as a fraction of 8 TB/s.
    python tools/mdct_probe.py [out.txt]        (default: profiles/r13_mdct.txt)"""
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hackathon_fft_amd as mf  # noqa: E402

DCT_SHAPES = [((100000, 1024), torch.float32), ((500000, 128), torch.float32), ((100000, 1024), torch.float64)]
MDCT_SHAPES = [((32, 480000), 256), ((32, 480000), 1024)]
PEAK = 8.0e12  # bytes / s
WINDOWS, CALLS, WARM = 7, 20, 5
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


def report(lines, label, t, nbytes, note):
    med, lo, hi = t
    frac = nbytes / (med * 1e-3) / PEAK
    lines.append(f"  {label:<26} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {nbytes / 1e6:9.1f} MB  {frac * 100:5.1f} % of 8 TB/s  {note}")
    print(lines[-1], flush=True)


def ratio(a, b):
    """median a / median b with the spread the run shows: [min a / max b .. max a / min b]"""
    return f"{a[0] / b[0]:.3f} [{a[1] / b[2]:.3f} .. {a[2] / b[1]:.3f}]"


def composed_dct4(x, ie, io, p):
    """DCT-IV from the pieces available without the tag: z = x[even] + i x[reversed odd], S = p fft(p z), interleave"""
    n = x.shape[-1]
    S = p * mf.fftn(torch.complex(x[:, ie], x[:, io]) * p)
    out = torch.empty_like(x)
    out[:, 0::2] = 2 * S.real
    out[:, n - 1 - 2 * torch.arange(n // 2, device=x.device)] = -2 * S.imag
    return out


def probe_dct4(lines):
    for shape, dtype in DCT_SHAPES:
        batch, n = shape
        esz = 4 if dtype == torch.float32 else 8
        lines.append(f"(a) {batch}x{n} {'fp32' if dtype == torch.float32 else 'fp64'}:")
        print(lines[-1], flush=True)
        x = torch.randn(shape + (1,), device=DEV, dtype=dtype)
        out = torch.empty_like(x)
        nbytes = 2 * batch * n * esz
        p4 = mf.plan_fft(dtype, dtype, x.shape, out.shape, dct=True, dct_type=4)
        p2 = mf.plan_fft(dtype, dtype, x.shape, out.shape, dct=True)
        x2 = x.squeeze(-1)
        ie = torch.arange(0, n, 2, device=DEV)
        io = n - 1 - ie
        m = torch.arange(n // 2, device=DEV, dtype=torch.float64)
        tw = torch.polar(torch.ones_like(m), -math.pi * (8 * m + 1) / (8 * n)).to(
            torch.complex64 if dtype == torch.float32 else torch.complex128)
        ref = mf.dct(x2[:64], type=4)
        err = ((composed_dct4(x2[:64], ie, io, tw) - ref).norm() / ref.norm()).item()
        ctx = mf.DeviceContext(0)
        t = measure({"dct4": lambda: mf.fft(out, x, ctx, plan=p4), "dct2": lambda: mf.fft(out, x, ctx, plan=p2),
                     "composition": lambda: composed_dct4(x2, ie, io, tw)})
        report(lines, "dct(type=4)", t["dct4"], nbytes, p4.kernel_name(0))
        report(lines, "dct(type=2)", t["dct2"], nbytes, p2.kernel_name(0))
        report(lines, "composition", t["composition"], nbytes,
               f"gather + twiddle + fftn + twiddle + scatter (agrees with dct(type=4) to {err:.1e})")
        lines.append(f"  ratios: type 4 / type 2 {ratio(t['dct4'], t['dct2'])}   composition / type 4 "
                     f"{ratio(t['composition'], t['dct4'])}")
        print(lines[-1], flush=True)
        del x, out, x2, p4, p2
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def probe_mdct(lines):
    dtype = torch.float32
    for (batch, T), n in MDCT_SHAPES:
        lines.append(f"(b) {batch}x{T} n={n} fp32:")
        print(lines[-1], flush=True)
        frames = mf.mdct_frames(T, n)
        x = torch.randn(batch, T, 1, device=DEV, dtype=dtype)
        plan = mf.plan_mdct(dtype, batch, T, n)
        out = torch.empty(plan.out_shape, device=DEV, dtype=dtype)
        nbytes = (batch * T + batch * frames * n) * 4
        w = mf.mdct_window(n).to(device=DEV, dtype=dtype)
        ia, sa, ib, sb = (t.to(DEV) for t in mf.api._mdct_fold_tables(n))
        sa, sb = sa.to(dtype), sb.to(dtype)
        x2 = x.squeeze(-1)

        def fold():
            y = F.pad(x2, (n, (frames + 1) * n - T - n)).unfold(-1, 2 * n, n) * w
            return (sa * y[..., ia] + sb * y[..., ib]).reshape(batch * frames, n)

        u = fold().unsqueeze(-1).contiguous()
        pf = mf.plan_fft(dtype, dtype, u.shape, u.shape, dct=True, dct_type=4)
        uo = torch.empty_like(u)
        ctx = mf.DeviceContext(0)
        mf.fft(out, x, ctx, plan=plan)
        err = ((mf.dct(fold(), type=4) / 2 - out.reshape(batch * frames, n)).norm() / out.norm()).item()
        t = measure({"mdct": lambda: mf.fft(out, x, ctx, plan=plan), "composition": lambda: mf.dct(fold(), type=4),
                     "floor": lambda: mf.fft(uo, u, ctx, plan=pf)})
        report(lines, "plan_mdct", t["mdct"], nbytes, f"{plan.kernel_name(1)} geometry={plan.pass_geometry(1)}")
        report(lines, "composition", t["composition"], nbytes,
               f"pad + unfold + window + fold + dct(type=4) (agrees with plan_mdct to {err:.1e})")
        report(lines, "floor: dct4 of folded rows", t["floor"], 2 * batch * frames * n * 4, pf.kernel_name(0))
        lines.append(f"  ratios: composition / mdct {ratio(t['composition'], t['mdct'])}   mdct / floor "
                     f"{ratio(t['mdct'], t['floor'])}")
        print(lines[-1], flush=True)
        del x, out, u, uo, plan, pf
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_mdct.txt")
    lines = [f"# tools/mdct_probe.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {WINDOWS} windows of {CALLS} "
             f"calls (HIP events), variants alternating, {WARM} warm-up calls each",
             "# bytes = x + out of the fused kernel, each moved once; fraction of 8 TB/s = bytes / median time / 8e12",
             "# ratio a / b = median a / median b [min a / max b .. max a / min b]"]
    probe_dct4(lines)
    probe_mdct(lines)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
