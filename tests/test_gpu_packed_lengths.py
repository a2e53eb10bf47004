"""One row length per configuration CLASS of the packed-row kernels, through every kernel of the family.

Ten public transforms -- one-sided rfftn / irfftn rows, dct / idct of types 2 and 4, stft, spectrogram, istft, mdct, imdct -- run
on packed_rows_config() -> choose_config(n / 2, rows) (csrc/kernels_jit.cpp), which derives from the half length N = n / 2 the
radix list, the rows per tile, the threads per workgroup, whether pass 0 prefetches and where the twiddle table lives; the load
and store loops of tile_kernel.h branch on N itself as well (odd N: a middle work item that is its own partner; even N: four
reals per access in the DCT-II rows; a single radix: one wave per workgroup).  The feature tests all run the same few lengths.
Here every class the function can produce gets one length, and every kernel runs at it against the fp64 numpy reference of its
own module, with that module's error measure, bounded by conftest's REL_L2_TOL_F32 / REL_L2_TOL_F64 and nothing else.
The families that came to ride on the same configuration function later -- the fused convolution and its filter gradient, the
gradients of stft and istft, the sine transforms -- go through the same table in tests/test_gpu_packed_families.py.

Every case asserts its class from the plan (radices from kernel_name, tile and threads from pass_geometry), writes into a
NaN-prefilled output with a NaN guard behind it, and finds its input unchanged.  The shapes hold two full tiles and a ragged
one (row kernels), or two batch entries whose frames straddle a tile (framed kernels)."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from istft_reference import istft_length, istft_reference, rel_l2_blocks, window_of
from test_dct4_host import ref_dct4
from test_gpu_dct import _rel, ref_dct, ref_idct
from test_gpu_imdct import _block_err, _coeffs
from test_gpu_imdct import _exec_guarded as imdct_exec
from test_gpu_imdct import _ref as imdct_ref
from test_gpu_imdct import _window as imdct_window
from test_gpu_istft import _device_spectrogram
from test_gpu_istft import _exec_guarded as istft_exec
from test_gpu_logmel import DB, check_elements, end_to_end, make_plan, uniform_fb
from test_gpu_mdct import _exec_guarded as mdct_exec
from test_gpu_mdct import _ref as mdct_ref
from test_gpu_mdct import _rel as frame_rel
from test_gpu_mdct import _window as mdct_window
from test_gpu_persistent_rounds import _as_rows, _bits, _cplx
from test_gpu_persistent_rounds import _exec_guarded as rows_exec
from test_gpu_spectrogram import _exec_guarded as spec_exec
from test_gpu_spectrogram import check, mel_fb, ref_and_bound
from test_gpu_stft import _exec_guarded as stft_exec
from test_gpu_stft import frame_err, hann, ref_stft

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
TOL = {"f32": REL_L2_TOL_F32, "f64": REL_L2_TOL_F64}
FAR = 1 << 40  # a count at which no grid is clamped by the tile count

# (dtype, n): (radices of N = n / 2, rows per tile, threads) -- what choose_config answers, and why the length is here.
# Where the twiddle table lives is not visible through a plan.  It follows from choose_config's byte count: the table stays in
# LDS while (N * tile + sum over the passes k >= 1 of P_k (R_k - 1)) complex elements fit 156 KiB (P_k: the product of the
# radices before pass k).  fp64 9600: (4800 + 4790) * 16 = 153440 bytes, in LDS; fp64 10000: (5000 + 4990) * 16 = 159840 bytes,
# 96 past 159744: global memory; fp64 12288: (6144 + 6120) * 16: global memory; every fp32 length here: in LDS.  The inverse
# STFT and the IMDCT count their carry (N, or N / 2, elements) too and move the table out earlier: both already at fp64 8192
# and 9600.
CLASSES = {
    ("f32", 14): ((7,), 64, 64),                  # odd prime N, one butterfly per row, one wave
    ("f32", 62): ((31,), 64, 64),                 # the largest single radix
    ("f32", 50): ((5, 5), 64, 256),               # odd N, two passes, tile at its cap
    ("f32", 192): ((12, 8), 42, 256),             # tile not a power of two
    ("f32", 2058): ((7, 7, 7, 3), 3, 256),        # odd N, four passes, small tile
    ("f32", 4802): ((7, 7, 7, 7), 1, 256),        # odd N, one row per workgroup
    ("f32", 10000): ((10, 10, 10, 5), 1, 512),    # one row, 512 threads
    ("f32", 12500): ((25, 25, 10), 1, 512),       # radix above 16: thread clamp, no prefetch
    ("f32", 12288): ((12, 8, 8, 8), 1, 1024),     # 1024 threads (prefetch in plain r2c), non-power-of-two radices
    ("f32", 13122): ((9, 9, 9, 9), 1, 1024),      # odd N at 1024 threads
    ("f64", 14): ((7,), 64, 64),                  # as f32
    ("f64", 66): ((11, 3), 62, 256),              # odd N, odd-sized tile, radix above the fp64 soft cap
    ("f64", 2058): ((7, 7, 7, 3), 1, 256),        # one row below the 2048-element budget
    ("f64", 4802): ((7, 7, 7, 7), 1, 512),        # odd N, 512 threads
    ("f64", 9600): ((10, 10, 8, 6), 1, 512),      # past 8192 points, table still in LDS
    ("f64", 10000): ((10, 10, 10, 5), 1, 512),    # table in global memory by 96 bytes
    ("f64", 12288): ((24, 16, 16), 1, 512),       # the longest fp64 row, radix 24, table in global memory
    # the two lengths only the overlap-adding kernels run (below): their carry shares the LDS
    ("f64", 8192): ((8, 8, 8, 8), 1, 512),        # ISTFT and IMDCT move the table to global memory from here
    ("f64", 10240): ((10, 8, 8, 8), 1, 512),      # the longest fp64 ISTFT: tile and carry are the CU's 160 KiB exactly
}
ONLY_OVERLAP_ADD = [("f64", 8192), ("f64", 10240)]
LENGTHS = [k for k in CLASSES if k not in ONLY_OVERLAP_ADD]
ISTFT_LENGTHS = [k for k in LENGTHS if k != ("f64", 12288)] + ONLY_OVERLAP_ADD  # (12288: tile and carry do not fit)
IMDCT_LENGTHS = LENGTHS + [("f64", 8192)]
SPEC_LENGTHS = [("f32", 14), ("f32", 2058), ("f32", 10000), ("f64", 10000)]


def _ids(v):
    return f"{v[0]}-{v[1]}" if isinstance(v, tuple) else str(v)


def _radices(name):
    """the radices in a kernel name: the field after r2c / c2r / dct2 / dct3 / dct4 / dst2 / dst3 / dst4"""
    parts = name.split("_")
    for i, p in enumerate(parts):
        if p in ("r2c", "c2r", "dct2", "dct3", "dct4", "dst2", "dst3", "dst4"):
            return tuple(int(v) for v in parts[i + 1].split("x"))
    raise AssertionError(name)


def _assert_class(plan, dim, t, n, threads_too):
    """the plan's pass over `dim` is the class the table names for (t, n); returns a text of kernel and geometry"""
    radices, tile, threads = CLASSES[(t, n)]
    name, geo = plan.kernel_name(dim), plan.pass_geometry(dim)
    text = f"{name} tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]}"
    assert name.startswith(f"rows{n}_" + ("f64_" if t == "f64" else "")), text
    assert _radices(name) == radices and int(np.prod(radices)) == n // 2, (text, radices)
    assert geo[0] == tile, (text, tile)
    if threads_too:
        assert geo[1] == threads, (text, threads)
    return text


def _report(kernel, t, n, err, text):
    print(f"packed-lengths {kernel} {t} n={n}: err {err:.3e} {text}")


# ---- row kernels: two full tiles and a ragged one -----------------------------------------------------------------------------

def _run_rows(kernel, t, n, make, in_shape, ref, norm=None):
    """kernel: the tag in the kernel's name; make(B) -> plan; in_shape(B); ref(x fp64 host) -> (B, m) float64"""
    tile = make(4).pass_geometry(0, FAR)[0]
    B = 2 * tile + max(1, tile // 3)
    plan = make(B)
    text = _assert_class(plan, 0, t, n, threads_too=True)
    assert f"_{kernel}_" in plan.kernel_name(0), text
    assert plan.pass_geometry(0)[2] == 3 and (tile == 1 or B % tile != 0), text
    xh = np.random.default_rng(n * 8 + len(kernel)).standard_normal(in_shape(B)).astype(NP[t])
    x = torch.from_numpy(xh).to(DEV)
    keep = x.clone()
    out = rows_exec(plan, x)
    assert torch.equal(_bits(x), _bits(keep)), "x was written"
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    err = _rel(_as_rows(out.cpu().numpy()), ref(xh.astype(np.float64)))
    _report(kernel + ("" if norm is None else "-" + norm), t, n, err, text)
    assert err <= TOL[t], (kernel, t, n, err, text)


@pytest.mark.parametrize("inverse", [False, True], ids=["r2c", "c2r"])
@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_half_spectrum_rows(tn, inverse):
    t, n = tn
    h = n // 2 + 1

    def shapes(b):
        real, half = (b, n, 1), (b, h, 2)
        return (half, real) if inverse else (real, half)

    make = lambda b: mf.plan_fft(DT[t], DT[t], *shapes(b), inverse=inverse, half_spectrum=True)
    if inverse:  # arbitrary complex bins: the imaginary parts of bins 0 and n / 2 are nonzero and must be ignored
        ref = lambda x: np.fft.irfft(_cplx(x), n=n, axis=-1)
    else:
        ref = lambda x: _as_rows(np.fft.rfft(x[..., 0], axis=-1))
    _run_rows("c2r" if inverse else "r2c", t, n, make, lambda b: shapes(b)[0], ref)


DCT_CASES = [(tn, None) for tn in LENGTHS] + [(("f32", 2058), "ortho")]


@pytest.mark.parametrize("kind", ["dct2", "dct3", "dct4"])
@pytest.mark.parametrize("tn,norm", DCT_CASES, ids=_ids)
def test_dct_rows(tn, norm, kind):
    t, n = tn
    make = lambda b: mf.plan_fft(DT[t], DT[t], (b, n, 1), (b, n, 1), inverse=kind == "dct3", dct=True, norm=norm,
                                 dct_type=4 if kind == "dct4" else 2)
    ref = {"dct2": lambda x: ref_dct(x[..., 0], norm), "dct3": lambda x: ref_idct(x[..., 0], norm),
           "dct4": lambda x: ref_dct4(x[..., 0], norm)}[kind]
    _run_rows(kind, t, n, make, lambda b: (b, n, 1), ref, norm)


# ---- framed kernels: two batch entries whose frames straddle a tile -----------------------------------------------------------

def _frames(tile):
    """frames per entry: with two entries, two full tiles and more, and no whole number of tiles per entry; one row per tile:
    three frames, so that a carry is handed on twice"""
    return tile + 1 if tile > 1 else 3


def _stft_shape(tile, n, hop):
    """(F, T) of a centred STFT entry: _frames(tile) or more, until one reflection reaches (T >= n / 2 + 1)"""
    F = _frames(tile)
    while (F - 1) * hop + hop // 2 < n // 2 + 1 or (tile > 1 and F % tile == 0):
        F += 1
    T = (F - 1) * hop + hop // 2
    assert mf.stft_frames(T, n, hop, True) == F and 2 * F >= 2 * tile + 1
    return F, T


@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_stft(tn):
    """periodic Hann, an odd hop (pair loads aligned to one element), centred by reflection"""
    t, n = tn
    B, hop, w = 2, (n // 4) | 1, hann(n)
    probe = mf.plan_stft(DT[t], 1, n, n, hop, window=w, center="reflect")
    tile = probe.pass_geometry(1, FAR)[0]
    probe.close()
    F, T = _stft_shape(tile, n, hop)
    plan = mf.plan_stft(DT[t], B, T, n, hop, window=w, center="reflect")
    text = _assert_class(plan, 1, t, n, threads_too=False)
    assert "_r2c_" in plan.kernel_name(1) and plan.kernel_name(1).endswith("_stft_jit"), text
    xh = np.random.default_rng(n + 1).standard_normal((B, T)).astype(NP[t])
    got = stft_exec(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    assert not np.isnan(got).any()
    err = frame_err(got, ref_stft(xh, n, hop, w, "reflect"))
    _report("stft", t, n, err, f"{text} B={B} T={T} F={F} hop={hop}")
    plan.close()
    assert err <= TOL[t], (t, n, err, text)


def _spec_banks(n):
    """(filterbank (K, M), post matrix (M, Q)): at 14 points all the n / 2 - 1 = 6 bands a post matrix allows, dense; else 40
    mel-style triangles"""
    K = n // 2 + 1
    if n == 14:
        return uniform_fb(K, 6, 14), np.random.default_rng(15).standard_normal((6, 3))
    return mel_fb(n, 40), np.random.default_rng(n).standard_normal((40, 13))


@pytest.mark.parametrize("store", ["p2", "p1_fb", "p2_fb_lg_pm"])
@pytest.mark.parametrize("tn", SPEC_LENGTHS, ids=_ids)
def test_spectrogram_stores(tn, store):
    """the three stores behind the STFT's passes: power, magnitude through a filterbank, and power through filterbank, decibels
    and a post matrix; frames as in test_stft"""
    t, n = tn
    dtype = DT[t]
    B, hop, w = 2, (n // 4) | 1, hann(n)
    fb, post = _spec_banks(n)
    power = 1 if store == "p1_fb" else 2
    kw = {"p2": {}, "p1_fb": dict(fb=fb), "p2_fb_lg_pm": dict(fb=fb, logv=DB, post=post)}[store]
    probe = make_plan(dtype, 1, n, n, hop, "reflect", w, power, **kw)
    tile = probe.pass_geometry(1, FAR)[0]
    probe.close()
    F, T = _stft_shape(tile, n, hop)
    plan = make_plan(dtype, B, T, n, hop, "reflect", w, power, **kw)
    text = _assert_class(plan, 1, t, n, threads_too=False)
    xh = np.random.default_rng(n + 2).standard_normal((B, T)).astype(NP[t])
    got = spec_exec(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1)).numpy().astype(np.float64)
    plan.close()
    what = f"packed-lengths spectrogram-{store} {t} n={n}: {text} B={B} T={T} F={F}"
    if store == "p2_fb_lg_pm":
        ref, bound = end_to_end(xh, dtype, n, hop, "reflect", 2, fb, DB, post)
        check_elements(got, ref, bound, what)
    else:
        ref, bound = ref_and_bound(ref_stft(xh, n, hop, w, "reflect"), power, kw.get("fb"), dtype)
        check(got, ref, bound, what)


@pytest.mark.parametrize("tn", ISTFT_LENGTHS, ids=_ids)
def test_istft(tn):
    """periodic Hann, hop n // 4, centred, `length` one sample short of the covered span: every entry ends ragged"""
    t, n = tn
    B, hop, w = 2, n // 4, window_of("hann", n)
    probe = mf.plan_istft(DT[t], 1, 2, n, hop, window=w, center=True)
    tile = probe.pass_geometry(2, FAR)[0]
    probe.close()
    F = _frames(tile)
    T = istft_length(F, n, hop, True) - 1
    Xh, X = _device_spectrogram(B, F, n, DT[t], seed=n + 3)
    plan = mf.plan_istft(DT[t], B, F, n, hop, window=w, center=True, length=T)
    text = _assert_class(plan, 2, t, n, threads_too=False)
    assert "_c2r_" in plan.kernel_name(2) and plan.kernel_name(2).endswith("_istft_jit"), text
    assert plan.pass_geometry(2)[2] == B * -(-F // tile) and (tile == 1 or F % tile != 0), text
    got = istft_exec(plan, X).cpu().numpy().reshape(B, T)
    assert not np.isnan(got).any()
    err = rel_l2_blocks(got, istft_reference(Xh, n, hop, w, True, T), hop)
    _report("istft", t, n, err, f"{text} B={B} F={F} hop={hop} T={T}")
    plan.close()
    assert err <= TOL[t], (t, n, err, text)


@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_mdct(tn):
    """n coefficients per frame of 2 n samples, a random window, T no multiple of n"""
    t, n = tn
    B, w = 2, mdct_window("random", n, n)
    probe = mf.plan_mdct(DT[t], 1, n, n, window=w)
    tile = probe.pass_geometry(1, FAR)[0]
    probe.close()
    F = _frames(tile)
    T = (F - 1) * n - n // 3
    assert mf.mdct_frames(T, n) == F and B * F >= 2 * tile + 1
    plan = mf.plan_mdct(DT[t], B, T, n, window=w)
    text = _assert_class(plan, 1, t, n, threads_too=False)
    assert "_dct4_" in plan.kernel_name(1) and plan.kernel_name(1).endswith("_mdct_jit"), text
    xh = np.random.default_rng(n + 4).standard_normal((B, T)).astype(NP[t])
    got = mdct_exec(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    assert not np.isnan(got).any()
    err = frame_rel(got, mdct_ref(xh, n, w, None))
    _report("mdct", t, n, err, f"{text} B={B} T={T} F={F}")
    plan.close()
    assert err <= TOL[t], (t, n, err, text)


@pytest.mark.parametrize("tn", IMDCT_LENGTHS, ids=_ids)
def test_imdct(tn):
    """uniform coefficients, a random window, length (F - 2) n + 1: the last block holds one sample"""
    t, n = tn
    B, w = 2, imdct_window("random", n)
    probe = mf.plan_imdct(DT[t], 1, 2, n, window=w)
    tile = probe.pass_geometry(2, FAR)[0]
    probe.close()
    F = _frames(tile)
    T = (F - 2) * n + 1
    Xh = _coeffs(B, F, n, DT[t], seed=5)
    plan = mf.plan_imdct(DT[t], B, F, n, length=T, window=w)
    text = _assert_class(plan, 2, t, n, threads_too=False)
    assert "_dct4_" in plan.kernel_name(2) and plan.kernel_name(2).endswith("_imdct_jit"), text
    assert plan.pass_geometry(2)[2] == B * -(-F // tile) and (tile == 1 or F % tile != 0), text
    got = imdct_exec(plan, torch.from_numpy(Xh).to(DEV).reshape(B, F, n, 1)).cpu().numpy()
    assert np.isfinite(got).all()
    err = _block_err(got, imdct_ref(Xh, n, w, None), n)
    _report("imdct", t, n, err, f"{text} B={B} F={F} T={T}")
    plan.close()
    assert err <= TOL[t], (t, n, err, text)
