"""What plan creation selects, for a fixed list of plans: one JSON record per case.

    python tools/plan_snapshot.py > tests/golden/plan_selection.json

Every plan of CASES is created on cuda:0 and asked what the introspection of the C ABI shows: the status (or the error status
and its message), num_launches, scratch_bytes and, per dim, kernel_name, stages and pass_geometry (or the status it raises).
Nothing is executed and no data tensor is allocated, so large shapes cost only the runtime compile of their kernels -- and
the plan scratch where a route needs one, which scratch_bytes records: the two rebuild cases allocate 1.07 GB and 0.92 GB
while their plan lives.

tests/test_gpu_plan_selection.py builds the same plans and asserts equality with the committed file, which was recorded at
the commit BEFORE the scheduler moved to csrc/schedule.cpp.  A change that alters selection on purpose regenerates the file
with this tool and says so; the expected values never come from the code under test.

The list covers every branch of the general route's scheduler (csrc/schedule.cpp) and each dispatched route once.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _fft(shape, real=False, dtype="float32", in_dtype=None, **kw):
    return ("fft", dict(shape=tuple(shape), real=real, dtype=dtype, in_dtype=in_dtype or dtype, **kw))


# id -> (kind, arguments).  The comment names the branch of the scheduler the shape takes.
CASES = {
    # table rows and runtime-specialised rows
    "c_16x1024": _fft((16, 1024)),
    "c_37x93": _fft((37, 93)),
    "c_9x343_jit": _fft((9, 343)),
    "r_i16_5x96": _fft((5, 96), real=True, in_dtype="int16"),
    # select_row2d, at any batch: it stands in front of the four-step that big batches prefer
    "c_3x16384_row2d": _fft((3, 16384)),
    "c_260x16384_row2d": _fft((260, 16384)),
    # the four-step preferred for a big batch (68 MB of 32768-point rows), and taken because the row is too long for one
    # workgroup (the product library's names do not tell the two apart); no split of 2^25 with both factors <= 4096: -9
    "c_260x32768_fourstep_preferred": _fft((260, 32768)),
    "c_3x32768_fourstep": _fft((3, 32768)),
    "c_3x100000_fourstep": _fft((3, 100000)),
    "c_1x2p25_bases2_too_large": _fft((1, 1 << 25), bases=[[2]]),
    # long strided dim: two column passes through the scratch
    "c_1x7680x64_fs_strided": _fft((1, 7680, 64)),
    # real 2-D: half-store pass in front of a Hermitian twin
    "r_25x640x480": _fft((25, 640, 480), real=True),
    "r_10x1920x1080": _fft((10, 1920, 1080), real=True),
    "r_f64_30x360x280": _fft((30, 360, 280), real=True, dtype="float64"),
    # the rounds rule of herm_pays: the wide twin cols64_8x8_w64_h does not pay (the narrow cols64_4x4x4_h is taken) / pays
    "r_1x64x64x64x64_wide_twin_declined": _fft((1, 64, 64, 64, 64), real=True),
    "r_4x64x64x64x64_wide_twin": _fft((4, 64, 64, 64, 64), real=True),
    # fused plane with half store
    "r_10x128x128x128": _fft((10, 128, 128, 128), real=True),
    "r_1x256x256x256": _fft((1, 256, 256, 256), real=True),
    "r_50x64x64x64": _fft((50, 64, 64, 64), real=True),
    # first-axis schedule: rows / columns / columns, plane / columns / columns
    "r_6x360x360x360_first_axis": _fft((6, 360, 360, 360), real=True),
    "r_2x64x64x64x64_first_axis": _fft((2, 64, 64, 64, 64), real=True),
    # the rebuild: the first-axis schedule started (on the plane; on the rows), abandoned at the end check because the long
    # middle dim takes more than one launch (transposed route; four-step through the scratch), the plan built again without it
    "r_1x8x4100x64x64_rebuild": _fft((1, 8, 4100, 64, 64), real=True),
    "r_2x32x5000x360_long_middle": _fft((2, 32, 5000, 360), real=True),
    # a streaming-size plan whose rows have a half-store table entry of their regime (rows1024_.._r_nt_hs): taken at once
    "r_64x1024x1024_hs_regime_entry": _fft((64, 1024, 1024), real=True),
    # ... and one whose rows have none (128 points): the regime twin rows128_.._r_nt is not traded for a runtime-specialised
    # half-store kernel (the `!tuned` of select_half_store; without it: rows128_16x8_hs_r_jit); the last pass is a twin anyway
    "r_1024x1024x128_regime_twin_kept": _fft((1024, 1024, 128), real=True),
    # complex N-D
    "c_100x640x480": _fft((100, 640, 480)),
    "c_10x128x128x128": _fft((10, 128, 128, 128)),
    # faithful_stages: the generic kernels
    "c_4x64x64_faithful": _fft((4, 64, 64), faithful_stages=True),
    # a slab selects as the whole batch does: names equal r_100x640x480's
    "r_100x640x480": _fft((100, 640, 480), real=True),
    "r_10x640x480_slab_of_100": _fft((10, 640, 480), real=True, whole_batch=100),
    # each dispatched route once
    "half_spectrum_fwd_3x640x480": ("half", dict(shape=(3, 640, 480), inverse=False)),
    "half_spectrum_inv_3x640x480": ("half", dict(shape=(3, 640, 480), inverse=True)),
    "axes2_4x32x48": _fft((4, 32, 48), axes=[2]),
    "dct2_8x64": ("dct", dict(shape=(8, 64), dct_type=2)),
    "dct4_8x64": ("dct", dict(shape=(8, 64), dct_type=4)),
    "dctn_4x32x32": ("dctn", dict(shape=(4, 32, 32))),
    "stft_3x160_n16_hop16": ("stft", dict(batch=3, length=160, n_fft=16, hop=16)),
    "spectrogram_4x1000_n64_hop16_fb8": ("spectrogram", dict(batch=4, length=1000, n_fft=64, hop=16, bands=8)),
    "istft_3x10_n16_hop16": ("istft", dict(batch=3, frames=10, n_fft=16, hop=16)),
    "mdct_3x1024_n64": ("mdct", dict(batch=3, length=1024, n=64)),
    "imdct_3x5_n64": ("imdct", dict(batch=3, frames=5, n=64)),
}


def make_plan(case_id: str):
    """the plan of one case (raises MifftError where plan creation refuses it)"""
    import torch

    import hackathon_fft_amd as mf

    kind, a = CASES[case_id]
    f32 = torch.float32
    if kind == "fft":
        dt, idt, shape = getattr(torch, a["dtype"]), getattr(torch, a["in_dtype"]), a["shape"]
        kw = {k: a[k] for k in ("bases", "faithful_stages", "whole_batch", "axes") if k in a}
        return mf.plan_fft(idt, dt, shape + (1 if a["real"] else 2,), shape + (2,), **kw)
    if kind == "half":
        shape = a["shape"]
        real, half = shape + (1,), shape[:-1] + (shape[-1] // 2 + 1, 2)
        return mf.plan_fft(f32, f32, half if a["inverse"] else real, real if a["inverse"] else half,
                           inverse=a["inverse"], half_spectrum=True)
    if kind == "dct":
        return mf.plan_fft(f32, f32, a["shape"] + (1,), a["shape"] + (1,), dct=True, dct_type=a["dct_type"])
    if kind == "dctn":
        return mf.plan_fft(f32, f32, a["shape"] + (1,), a["shape"] + (1,), dctn=True)
    if kind == "stft":
        return mf.plan_stft(f32, a["batch"], a["length"], a["n_fft"], a["hop"])
    if kind == "spectrogram":
        bins, bands = a["n_fft"] // 2 + 1, a["bands"]  # (band m: the bins m, m + bands, ..)
        fb = (torch.arange(bins)[:, None] % bands == torch.arange(bands)[None, :]).to(torch.float64)
        return mf.plan_spectrogram(f32, a["batch"], a["length"], a["n_fft"], a["hop"], power=2, fb=fb)
    if kind == "istft":
        return mf.plan_istft(f32, a["batch"], a["frames"], a["n_fft"], a["hop"])
    if kind == "mdct":
        return mf.plan_mdct(f32, a["batch"], a["length"], a["n"])
    if kind == "imdct":
        return mf.plan_imdct(f32, a["batch"], a["frames"], a["n"])
    raise KeyError(kind)


def snapshot(case_id: str) -> dict:
    """the record of one case, in the form the committed file holds"""
    from hackathon_fft_amd import MifftError

    try:
        plan = make_plan(case_id)
    except MifftError as e:
        return {"status": e.status, "message": e.message}
    dims = []
    for d in range(plan.ndim):
        try:
            geometry = list(plan.pass_geometry(d))
        except MifftError as e:
            geometry = {"status": e.status}
        dims.append({"kernel_name": plan.kernel_name(d), "stages": plan.stages(d), "pass_geometry": geometry})
    rec = {"status": 0, "num_launches": plan.num_launches, "scratch_bytes": plan.scratch_bytes, "dims": dims}
    plan.close()
    return rec


def main() -> int:
    ids = sys.argv[1:] or list(CASES)
    print(json.dumps({i: snapshot(i) for i in ids}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
