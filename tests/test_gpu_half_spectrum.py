"""Half-spectrum real transforms on the MI355X (MIFFT_FLAG_HALF_SPECTRUM): the packed real-row kernels (TileCfg::R2C
forward, TileCfg::C2R inverse) and the column passes over the n // 2 + 1 bins, against numpy's rfftn / irfftn in fp64."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT, REL_L2_TOL_F32, REL_L2_TOL_F64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _rel(got, ref):
    """max over the batch of ||got - ref|| / ||ref|| (complex or real arrays, leading axis = batch)"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.complex128 if np.iscomplexobj(got) else np.float64).reshape(b, -1)
    r = np.asarray(ref).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _forward(x_np, dtype, in_dtype=None):
    """one-sided forward through a Plan: NaN-prefilled output, x checked unchanged; returns (complex result, plan)"""
    in_dtype = in_dtype or dtype
    xd = torch.from_numpy(np.ascontiguousarray(x_np)).to(DEV).to(in_dtype).unsqueeze(-1).contiguous()
    keep = xd.clone()
    shape = tuple(xd.shape)
    out_shape = shape[:-2] + (shape[-2] // 2 + 1, 2)
    out = torch.full(out_shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(in_dtype, dtype, shape, out_shape, half_spectrum=True)
    mf.fft(out, xd, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    o = out.cpu().numpy().astype(np.float64)
    assert not np.isnan(o).any()
    return o[..., 0] + 1j * o[..., 1], plan


def _inverse(X_np, dtype, n):
    Xr = np.stack([X_np.real, X_np.imag], axis=-1).astype(NP[dtype])
    xd = torch.from_numpy(Xr).to(DEV)
    keep = xd.clone()
    out_shape = tuple(xd.shape[:-2]) + (n, 1)
    out = torch.full(out_shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(dtype, dtype, tuple(xd.shape), out_shape, inverse=True, half_spectrum=True)
    mf.fft(out, xd, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    o = out.cpu().numpy()[..., 0].astype(np.float64)
    assert not np.isnan(o).any()
    return o, plan


def _axes(x):
    return tuple(range(1, x.ndim))


# (shape incl. batch, fp64 too?) -- batches leave ragged row tiles and column tiles
SHAPES_1D = [((37, 8), True), ((29, 16), False), ((33, 128), True), ((21, 480), True), ((19, 1024), True),
             ((13, 1080), False), ((5, 1920), True), ((11, 686), True),  # 686 = 2 * 7^3: odd packed length, hipRTC
             ((3, 8192), True)]  # (the longest fp64 power of two)
SHAPES_ND = [((3, 640, 480), True), ((2, 1920, 1080), False), ((3, 64, 64, 64), True), ((1, 128, 128, 128), False),
             ((1, 25, 160, 160, 48), False)]
CASES = [(s, torch.float32) for s, _ in SHAPES_1D + SHAPES_ND] + \
        [(s, torch.float64) for s, f64 in SHAPES_1D + SHAPES_ND if f64]


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_forward_matches_numpy_rfftn(shape, dtype):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(NP[dtype])
    got, plan = _forward(x, dtype)
    ref = np.fft.rfftn(x.astype(np.float64), axes=_axes(x))
    assert got.shape == ref.shape
    err = _rel(got, ref)
    assert err <= TOL[dtype], (shape, err, [plan.kernel_name(d) for d in range(plan.ndim)])


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_inverse_matches_numpy_irfftn_on_arbitrary_input(shape, dtype):
    """X is NOT the spectrum of a real tensor: the imaginary parts of bins 0 and n / 2 are nonzero, as everywhere"""
    rng = np.random.default_rng(sum(shape) + 1)
    n = shape[-1]
    hshape = shape[:-1] + (n // 2 + 1,)
    X = (rng.standard_normal(hshape) + 1j * rng.standard_normal(hshape)).astype(np.complex128)
    X = X.astype(np.complex64 if dtype == torch.float32 else np.complex128).astype(np.complex128)
    got, plan = _inverse(X, dtype, n)
    ref = np.fft.irfftn(X, s=shape[1:], axes=_axes(X))
    err = _rel(got, ref)
    assert err <= TOL[dtype], (shape, err, [plan.kernel_name(d) for d in range(plan.ndim)])


@pytest.mark.parametrize("shape", [(5, 480), (3, 1080), (2, 640, 480), (2, 64, 64, 64)], ids=str)
def test_round_trip(shape):
    x = torch.randn(shape, device=DEV)
    X = mf.rfftn(x, onesided=True)
    assert X.shape == shape[:-1] + (shape[-1] // 2 + 1,) and X.dtype == torch.complex64
    y = mf.irfftn(X, n=shape[-1])
    assert y.shape == x.shape and y.dtype == torch.float32
    assert _rel(y.cpu().numpy(), x.cpu().numpy()) <= 1e-5
    Xd = torch.view_as_real(X)  # interleaved input, default n
    assert _rel(mf.irfftn(Xd).cpu().numpy(), x.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.int16, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", [(9, 480), (2, 64, 96)], ids=str)
def test_narrow_input_types_are_widened(in_dtype, shape):
    rng = np.random.default_rng(7)
    if in_dtype == torch.uint8:
        xt = torch.from_numpy(rng.integers(0, 256, size=shape).astype(np.uint8))
    elif in_dtype == torch.int16:
        xt = torch.from_numpy(rng.integers(-30000, 30000, size=shape).astype(np.int16))
    else:
        xt = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(in_dtype)
    wide = xt.to(torch.float64).numpy()
    src = xt.numpy() if in_dtype in (torch.uint8, torch.int16) else xt.float().numpy()  # (exact in float32)
    got, plan = _forward(src, torch.float32, in_dtype=in_dtype)
    assert plan.in_dtype == in_dtype
    err = _rel(got, np.fft.rfftn(wide, axes=_axes(wide)))
    assert err <= REL_L2_TOL_F32, err


@pytest.mark.parametrize("shape", [(7, 1024), (3, 640, 480), (2, 64, 64, 64)], ids=str)
def test_agrees_with_the_full_spectrum_route(shape):
    x = torch.randn(shape, device=DEV)
    full = mf.rfftn(x)  # today's full-spectrum real plan, interleaved
    half = torch.view_as_real(mf.rfftn(x, onesided=True))
    h = shape[-1] // 2 + 1
    ref = full[..., :h, :].cpu().numpy()
    assert _rel(half.cpu().numpy(), ref) <= 1e-5


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape", [(10, 480), (6, 48, 40), (5, 16, 24, 32)], ids=str)
def test_slabs_are_bit_identical(shape, inverse):
    n, batch = shape[-1], shape[0]
    h = n // 2 + 1
    if inverse:
        in_shape, out_shape = shape[:-1] + (h, 2), shape + (1,)
    else:
        in_shape, out_shape = shape + (1,), shape[:-1] + (h, 2)
    x = torch.randn(in_shape, device=DEV)
    plan = mf.plan_fft(torch.float32, torch.float32, in_shape, out_shape, inverse=inverse, half_spectrum=True)
    whole = torch.full(out_shape, float("nan"), device=DEV)
    mf.fft(whole, x, plan=plan)
    parts = torch.full(out_shape, float("nan"), device=DEV)
    for first, count in ((0, 3), (3, 1), (4, batch - 4)):
        mf.fft(parts, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    # a plan over one slab, sized for the whole batch
    s_in, s_out = (4,) + in_shape[1:], (4,) + out_shape[1:]
    slab = mf.plan_fft(torch.float32, torch.float32, s_in, s_out, inverse=inverse, half_spectrum=True,
                       whole_batch=batch)
    got = torch.full(s_out, float("nan"), device=DEV)
    mf.fft(got, x[1:5].contiguous(), plan=slab)
    torch.cuda.synchronize()
    assert torch.equal(got, whole[1:5])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape", [(4, 1024), (3, 640, 480), (2, 64, 64, 64)], ids=str)
def test_introspection(shape, dtype):
    esz = 4 if dtype == torch.float32 else 8
    n, batch, nd = shape[-1], shape[0], len(shape) - 1
    h = n // 2 + 1
    H = int(np.prod(shape[1:-1])) * h
    real = int(np.prod(shape[1:]))
    fwd = mf.plan_fft(dtype, dtype, shape + (1,), shape[:-1] + (h, 2), half_spectrum=True)
    assert fwd.in_bytes == batch * real * esz
    assert fwd.out_bytes == batch * H * 2 * esz
    assert fwd.scratch_bytes == 0 and fwd.num_launches == nd
    assert "_r2c_" in fwd.kernel_name(nd - 1), fwd.kernel_name(nd - 1)
    inv = mf.plan_fft(dtype, dtype, shape[:-1] + (h, 2), shape + (1,), inverse=True, half_spectrum=True)
    assert inv.in_bytes == batch * H * 2 * esz
    assert inv.out_bytes == batch * real * esz
    assert inv.scratch_bytes == (batch * H * 2 * esz if nd >= 2 else 0)
    assert inv.num_launches == nd
    assert "_c2r_" in inv.kernel_name(nd - 1), inv.kernel_name(nd - 1)
    for d in range(nd - 1):
        assert inv.kernel_name(d).startswith("cols"), inv.kernel_name(d)


def _create(dims, *, comps, inverse, flags=2, in_dtype=0, out_dtype=0):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, len(dims), c_dims, 2, comps, int(inverse), None,
                             None, flags)
    why = L.mifft_last_error().decode()
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, why


@pytest.mark.parametrize("inverse", [False, True])
def test_unsupported_requests_are_refused_with_a_reason(inverse):
    comps = 2 if inverse else 1
    for dims, flags in (([32, 45], 2), ([64, 32], 3), ([4100, 16], 2), ([2 * 37], 2), ([32768], 2),
                        ([6], 2)):
        rc, why = _create(dims, comps=comps, inverse=inverse, flags=flags)
        assert rc == -15 and why, (dims, flags, rc, why)
    assert _create([64, 32], comps=comps, inverse=inverse)[0] == 0
    assert _create([64, 32], comps=3 - comps, inverse=inverse)[0] == -3


def test_without_runtime_specialisation_the_precompiled_lengths_plan():
    """MIFFT_JIT=0 (a fresh process): the BASELINE / reference-bench last dims plan on precompiled packed-row kernels, fp32
    and fp64, both directions; a length without an instance is refused with the reason."""
    code = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from hackathon_fft_amd import _lib\n"
            "L = _lib.lib()\n"
            "for n in (128, 480, 1024, 1080, 1920, 1000):\n"
            "    for dt in (0, 1):\n"
            "        for inv in (0, 1):\n"
            "            h = ctypes.c_void_p(); d = (ctypes.c_int64 * 1)(n)\n"
            "            rc = L.mifft_plan_create(ctypes.byref(h), 0, dt, dt, 1, d, 4, 1 + inv, inv, None, None, 2)\n"
            "            name = L.mifft_plan_kernel_name(h, 0).decode() if rc == 0 else L.mifft_last_error().decode()\n"
            "            if rc == 0: L.mifft_plan_destroy(h)\n"
            "            print(n, dt, inv, rc, name)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 24
    for ln in lines:
        n, dt, inv, rc, name = ln.split(" ", 4)
        if n == "1000":
            assert int(rc) == -15 and "MIFFT_JIT=0" in name, ln
        else:
            assert int(rc) == 0, ln
            assert ("_c2r_" if inv == "1" else "_r2c_") in name and not name.endswith("_jit"), ln


def test_cache_resident_plans_take_the_streaming_load_twin():
    """a 2-D forward whose half spectrum fits the Infinity-Cache window reads x with non-temporal loads (`_ntl`)"""
    shape = (140, 640, 480)  # 140 * 640 * 241 complex64 = 173 MB
    x = torch.randn(shape, device=DEV)
    X = mf.rfftn(x, onesided=True)
    plan = mf.plan_fft(torch.float32, torch.float32, shape + (1,), shape[:-1] + (241, 2), half_spectrum=True)
    assert plan.kernel_name(1).endswith("_ntl"), plan.kernel_name(1)
    small = mf.plan_fft(torch.float32, torch.float32, (2, 640, 480, 1), (2, 640, 241, 2), half_spectrum=True)
    assert not small.kernel_name(1).endswith("_ntl"), small.kernel_name(1)
    rows = [0, 77, 139]
    ref = np.fft.rfftn(x[rows].double().cpu().numpy(), axes=(1, 2))
    assert _rel(X[rows].cpu().numpy(), ref) <= REL_L2_TOL_F32
