"""Transforms over a subset of the dims on the MI355X (MIFFT_FLAG_KEEP_DIM, torch `dim=`): the interleaved block tile
(TileCfg::ILV) for small kept strides, the column tiles reading x out of place, the literal-stage fallback, half spectra
with kept dims and the wrappers' `dim` argument, against numpy.fft in fp64."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import ROOT, REL_L2_TOL_F32, REL_L2_TOL_F64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
ESZ = {torch.float32: 8, torch.float64: 16}


def _rel(got, ref):
    """max over the batch of ||got - ref|| / ||ref|| (leading axis = batch)"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.complex128 if np.iscomplexobj(got) else np.float64).reshape(b, -1)
    r = np.asarray(ref).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _run_plan(x_np, axes, dtype, *, inverse=False, in_dtype=None, whole_batch=0):
    """x_np: (batch, d0.., C) in the layout; NaN-prefilled output, x checked unchanged; returns (complex result, plan)"""
    in_dtype = in_dtype or dtype
    xd = torch.from_numpy(np.ascontiguousarray(x_np)).to(DEV).to(in_dtype)
    keep = xd.clone()
    out_shape = tuple(xd.shape[:-1]) + (2,)
    out = torch.full(out_shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(in_dtype, dtype, tuple(xd.shape), out_shape, inverse=inverse, axes=axes, whole_batch=whole_batch)
    mf.fft(out, xd, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    o = out.cpu().numpy().astype(np.float64)
    assert not np.isnan(o).any()
    return o[..., 0] + 1j * o[..., 1], plan


def _cplx(rng, shape, dtype):
    x = rng.standard_normal(shape + (2,)).astype(NP[dtype])
    return x, x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("N", [93, 128, 480, 1024])
@pytest.mark.parametrize("I", [2, 3, 5, 8, 15, 16, 17, 100])
def test_kept_trailing_stride(I, N, dtype):
    """(B, N, I) with dim 1 transformed: the interleaved tile below 128 B of kept elements, the column tiles from there"""
    rng = np.random.default_rng(I * 1000 + N)
    B = 3
    x, xc = _cplx(rng, (B, N, I), dtype)
    for inverse in (False, True):
        got, plan = _run_plan(x, (1,), dtype, inverse=inverse)
        ref = (np.fft.ifftn if inverse else np.fft.fftn)(xc, axes=(1,))
        err = _rel(got, ref)
        name = plan.kernel_name(0)
        assert err <= TOL[dtype], (I, N, dtype, inverse, name, err)
        assert plan.kernel_name(1) == "none" and plan.stages(1) == [] and plan.num_launches == 1
        if I * ESZ[dtype] < 128:
            assert name.startswith(f"ilv{N}x{I}_"), name
        else:
            assert not name.startswith("ilv"), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kept_middle_and_leading_dims(dtype):
    rng = np.random.default_rng(7)
    x, xc = _cplx(rng, (3, 64, 7, 64), dtype)
    for inverse in (False, True):
        got, plan = _run_plan(x, (1, 3), dtype, inverse=inverse)
        ref = (np.fft.ifftn if inverse else np.fft.fftn)(xc, axes=(1, 3))
        assert _rel(got, ref) <= TOL[dtype], plan.kernel_name(0)
        assert plan.num_launches == 2 and plan.kernel_name(1) == "none"
    # kept leading dims: a (2, 5, 6, 96) tensor, only the last two transformed -> the wrappers fold (2, 5) into the batch
    xt = torch.from_numpy(rng.standard_normal((2, 5, 6, 96)) + 1j * rng.standard_normal((2, 5, 6, 96))).to(DEV)
    xt = xt.to(torch.complex64 if dtype == torch.float32 else torch.complex128)
    got = mf.fftn(xt, dim=(-2, -1)).cpu().numpy()
    ref = np.fft.fftn(xt.cpu().numpy().astype(np.complex128), axes=(2, 3))
    assert _rel(got.reshape(10, -1), ref.reshape(10, -1)) <= TOL[dtype]
    # dim 0 transformed, dim 1 kept
    got = mf.ifftn(xt, dim=(0, 3)).cpu().numpy()
    ref = np.fft.ifftn(xt.cpu().numpy().astype(np.complex128), axes=(0, 3))
    assert _rel(got[None], ref[None]) <= TOL[dtype]


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.uint8, torch.int16, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("comps", [1, 2])
def test_first_pass_reads_real_and_foreign_input_at_a_stride(in_dtype, comps):
    """kept innermost dim: the first (and only) pass is strided and reads x with its element type and component count"""
    rng = np.random.default_rng(comps * 10 + 3)
    for shape, I in (((4, 480, 4), 4), ((4, 128, 24), 24)):  # interleaved tile, column tile
        if in_dtype == torch.uint8:
            x = rng.integers(0, 255, size=shape + (comps,)).astype(np.float64)
        elif in_dtype == torch.int16:
            x = rng.integers(-3000, 3000, size=shape + (comps,)).astype(np.float64)
        else:
            x = rng.standard_normal(shape + (comps,))
        xt = torch.from_numpy(x).to(in_dtype)
        xv = xt.double().numpy()  # the values the plan sees
        xc = xv[..., 0] + (1j * xv[..., 1] if comps == 2 else 0)
        got, plan = _run_plan(xt.numpy() if in_dtype not in (torch.bfloat16,) else xt.float().numpy(), (1,),
                              torch.float32, in_dtype=in_dtype)
        ref = np.fft.fftn(xc, axes=(1,))
        assert _rel(got, ref) <= REL_L2_TOL_F32, (in_dtype, comps, shape, plan.kernel_name(0))
        if I == 4:
            assert plan.kernel_name(0).startswith("ilv480x4_"), plan.kernel_name(0)


@pytest.mark.parametrize("shape,axes", [((3, 97, 4), (1,)), ((3, 4096, 8), (1,)), ((2, 97, 6, 4), (1, 3))])
def test_fallback_routes(shape, axes):
    """a Rader length (97) and a block beyond the tile's LDS (4096 x 8 fp32 = 256 KiB) take the column tiles"""
    rng = np.random.default_rng(97)
    x, xc = _cplx(rng, shape, torch.float32)
    got, plan = _run_plan(x, axes, torch.float32)
    ref = np.fft.fftn(xc, axes=axes)
    assert _rel(got, ref) <= REL_L2_TOL_F32, plan.kernel_name(axes[0] - 1)
    assert not plan.kernel_name(0).startswith("ilv"), plan.kernel_name(0)


def test_wrapper_matches_torch_fft():
    x = torch.randn(4, 40, 30, 3, dtype=torch.complex64, device=DEV)
    for dim in ((1, 2), 1, (-1,), (0, 2), (3, 1)):
        got = mf.fftn(x, dim=dim)
        ref = torch.fft.fftn(x, dim=dim)
        err = ((got - ref).abs().pow(2).sum() / ref.abs().pow(2).sum()).sqrt().item()
        assert err <= 1e-5, (dim, err)
        back = mf.ifftn(got, dim=dim)
        assert ((back - x).abs().max() <= 1e-4).item(), dim
    assert torch.equal(mf.fftn(x, dim=()), x)  # nothing to transform: a converted copy


def test_all_but_first_is_bit_identical_to_the_plain_call():
    x = torch.randn(8, 64, 96, dtype=torch.complex64, device=DEV)
    assert torch.equal(mf.fftn(x, dim=(1, 2)), mf.fftn(x))
    assert torch.equal(mf.ifftn(x, dim=(-2, -1)), mf.ifftn(x))
    r = torch.randn(8, 64, 96, device=DEV)
    assert torch.equal(mf.rfftn(r, dim=(1, 2), onesided=True), mf.rfftn(r, onesided=True))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_half_spectrum_with_a_kept_middle_dim(dtype):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 16, 5, 32)).astype(NP[dtype])
    xt = torch.from_numpy(x).to(DEV)
    X = mf.rfftn(xt, dim=(1, 3), onesided=True)
    ref = np.fft.rfftn(x.astype(np.float64), axes=(1, 3))
    assert tuple(X.shape) == (3, 16, 5, 17)
    assert _rel(X.cpu().numpy(), ref) <= TOL[dtype]
    back = mf.irfftn(X, dim=(1, 3))
    refb = np.fft.irfftn(ref, s=(16, 32), axes=(1, 3))
    assert _rel(back.cpu().numpy(), refb) <= TOL[dtype]
    assert _rel(back.cpu().numpy(), x.astype(np.float64)) <= TOL[dtype]
    # only the innermost dim transformed: the packed rows alone
    X1 = mf.rfftn(xt, dim=3, onesided=True)
    assert _rel(X1.cpu().numpy(), np.fft.rfftn(x.astype(np.float64), axes=(3,))) <= TOL[dtype]
    with pytest.raises(mf.MifftError) as e:  # the innermost dim kept: refused
        mf.rfftn(xt, dim=(1, 2), onesided=True)
    assert e.value.status == -15


def test_slab_plans_with_a_mask_equal_the_whole_batch():
    rng = np.random.default_rng(5)
    x, _ = _cplx(rng, (12, 480, 4), torch.float32)
    whole, _ = _run_plan(x, (1,), torch.float32)
    for a, b in ((0, 5), (5, 12)):
        part, plan = _run_plan(x[a:b], (1,), torch.float32, whole_batch=12)
        assert np.array_equal(part, whole[a:b]), (a, b, plan.kernel_name(0))


def test_without_runtime_specialisation_a_kept_innermost_plan_runs():
    """MIFFT_JIT=0 (a fresh process): no interleaved tile, a tuned column tile or the literal stages instead"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np, torch, hackathon_fft_amd as mf\n"
            "rng = np.random.default_rng(3)\n"
            "for shape in ((3, 480, 4), (3, 93, 2), (3, 343, 5)):\n"
            "    x = rng.standard_normal(shape + (2,)).astype(np.float32)\n"
            "    xd = torch.from_numpy(x).to('cuda:0'); out = torch.full_like(xd, float('nan'))\n"
            "    plan = mf.plan_fft(torch.float32, torch.float32, xd.shape, xd.shape, axes=(1,))\n"
            "    mf.fft(out, xd, plan=plan); torch.cuda.synchronize()\n"
            "    o = out.cpu().numpy().astype(np.float64); g = o[..., 0] + 1j * o[..., 1]\n"
            "    r = np.fft.fftn(x[..., 0].astype(np.float64) + 1j * x[..., 1], axes=(1,))\n"
            "    err = float(np.linalg.norm(g - r) / np.linalg.norm(r))\n"
            "    print(shape[1], plan.kernel_name(0), err, bool(np.isnan(o).any()))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3, r.stdout
    for ln in lines:
        n, name, err, nan = ln.split(" ")
        assert nan == "False" and float(err) <= REL_L2_TOL_F32, ln
        assert not name.startswith("ilv") and not name.endswith("_jit"), ln
