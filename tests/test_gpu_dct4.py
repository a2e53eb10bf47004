"""DCT-IV of real rows on the MI355X (MIFFT_DCT_TYPE4_TAG): the TileCfg::DCT = 4 kernel against the fp64 numpy references of
test_dct4_host.py -- the cosine matrix up to 1080 points, the n / 2-point complex route beyond (checked against the matrix there)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import ROOT, REL_L2_TOL_F32, REL_L2_TOL_F64
from test_dct4_host import dct4_matrix, ref_dct4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]


def _rel(got, ref):
    """max over the rows of ||got - ref|| / ||ref|| (real arrays, leading axis = batch)"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.float64).reshape(b, -1)
    r = np.asarray(ref, dtype=np.float64).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _run(x_np, dtype, *, inverse, norm=None, first=None, count=None):
    """through a Plan: NaN-prefilled output, x checked unchanged; returns (fp64 result, plan)"""
    xd = torch.from_numpy(np.ascontiguousarray(x_np)).to(DEV).to(dtype).unsqueeze(-1).contiguous()
    keep = xd.clone()
    shape = tuple(xd.shape)
    out = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(dtype, dtype, shape, shape, inverse=inverse, dct=True, dct_type=4, norm=norm)
    if first is None:
        mf.fft(out, xd, plan=plan)
    else:
        mf.fft(out, xd, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    return out.cpu().numpy()[..., 0].astype(np.float64), plan


# (batch, n), fp64 too? -- odd batches leave ragged row tiles
SHAPES = [((37, 8), True),      # N = 4
          ((29, 16), True),
          ((23, 30), True),     # N = 15: the middle work item is its own partner
          ((21, 480), True),
          ((19, 1024), True),
          ((11, 686), True),    # N = 343
          ((3, 8192), True),    # the longest fp64 power of two
          ((2, 16384), False)]  # the longest row
CASES = [(s, torch.float32) for s, _ in SHAPES] + [(s, torch.float64) for s, f64 in SHAPES if f64]


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("inverse", [False, True], ids=["dct", "idct"])
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_both_directions_match_the_reference(shape, dtype, inverse, norm):
    rng = np.random.default_rng(sum(shape) + int(inverse))
    x = rng.standard_normal(shape).astype(NP[dtype])
    got, plan = _run(x, dtype, inverse=inverse, norm=norm)
    assert not np.isnan(got).any()
    err = _rel(got, ref_dct4(x, norm, inverse))
    name = plan.kernel_name(0)
    print(f"{'idct' if inverse else 'dct'}4 {shape} {dtype} norm={norm}: rel L2 {err:.3e} {name}")
    assert err <= TOL[dtype], (shape, err, name)
    n = shape[1]
    assert name.startswith(f"rows{n}_" + ("f64_" if dtype == torch.float64 else "") + "dct4_") and name.endswith("_jit"), name
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert int(np.prod(plan.stages(0))) == n // 2
    esz = 4 if dtype == torch.float32 else 8
    assert plan.in_bytes == plan.out_bytes == shape[0] * n * esz


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [30, 1024])
def test_structured_input_bin_by_bin(n, dtype):
    """unit impulses at both ends and both sides of the middle, and a constant row: an index slip in the paired load or store
    would hide inside an L2 norm.  A unit impulse has a transform of norm sqrt(2n): the absolute tolerance is TOL sqrt(n)."""
    tol = TOL[dtype]
    where = [0, 1, n // 2 - 1, n // 2, n - 2, n - 1]
    x = np.zeros((len(where) + 1, n), dtype=NP[dtype])
    for row, j in enumerate(where):
        x[row, j] = 1.0
    c = 0.75
    x[-1, :] = c
    got, _ = _run(x, dtype, inverse=False)
    assert not np.isnan(got).any()
    k = np.arange(n)
    for row, j in enumerate(where):
        want = 2 * np.cos(np.pi * (2 * j + 1) * (2 * k + 1) / (4 * n))
        assert np.abs(got[row] - want).max() <= tol * np.sqrt(n), (row, j, np.abs(got[row] - want).argmax())
    want = c * (-1.0) ** k / np.sin(np.pi * (2 * k + 1) / (4 * n))  # 2 c sum_j cos(..): peak 4 n c / pi at k = 0
    assert np.abs(want - x[-1].astype(np.float64) @ dct4_matrix(n)).max() < 1e-9
    assert np.abs(got[-1] - want).max() <= tol * np.abs(want).max(), np.abs(got[-1] - want).argmax()
    # the inverse of unit coefficients: the same cosines over 2n
    back, _ = _run(x[:-1], dtype, inverse=True)
    for row, kk in enumerate(where):
        want = 2 * np.cos(np.pi * (2 * kk + 1) * (2 * k + 1) / (4 * n)) / (2 * n)
        assert np.abs(back[row] - want).max() <= tol * np.sqrt(n) / (2 * n), (row, kk)


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape", [(7, 30), (5, 480), (4, 1024)], ids=str)
def test_round_trips(shape, dtype, norm):
    tol = TOL[dtype]
    x = torch.randn(shape, dtype=dtype, device=DEV)
    X = mf.dct(x, type=4, norm=norm)
    assert X.shape == x.shape and X.dtype == dtype
    xn, Xn = x.cpu().numpy(), X.cpu().numpy()
    assert _rel(Xn, ref_dct4(xn, norm)) <= tol
    assert _rel(mf.idct(X, type=4, norm=norm).cpu().numpy(), xn) <= tol
    assert _rel(mf.dct(mf.idct(x, type=4, norm=norm), type=4, norm=norm).cpu().numpy(), xn) <= tol
    if norm == "ortho":  # an involution, and Parseval
        assert _rel(mf.dct(X, type=4, norm="ortho").cpu().numpy(), xn) <= tol
        assert torch.equal(mf.idct(x, type=4, norm="ortho"), X)  # (the same kernel with the same scale)
        nx, nX = np.linalg.norm(xn.astype(np.float64), axis=1), np.linalg.norm(Xn.astype(np.float64), axis=1)
        assert (np.abs(nX - nx) <= tol * nx).all()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [30, 1024])
def test_a_middle_slab_equals_the_same_rows_of_the_whole_batch(n, inverse):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((11, n)).astype(np.float32)
    whole, _ = _run(x, torch.float32, inverse=inverse)
    part, _ = _run(x, torch.float32, inverse=inverse, first=3, count=5)
    assert np.array_equal(part[3:8], whole[3:8])
    assert np.isnan(part[:3]).all() and np.isnan(part[8:]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_base_pointer_aligned_to_one_element_only(offset, dtype):
    """contiguous slices at a storage offset of 1 .. 3 elements, on both sides: the kernel's pair accesses are then aligned to
    one element only, the contract of include/mifft.h"""
    n, rows = 64, 5
    big = torch.randn(offset + rows * n, dtype=dtype, device=DEV)
    x = big[offset:].reshape(rows, n, 1)
    assert x.is_contiguous() and x.data_ptr() % (4 * x.element_size()) != 0
    xn = x[..., 0].cpu().numpy()
    for inverse in (False, True):
        obig = torch.full((offset + rows * n + 8,), float("nan"), dtype=dtype, device=DEV)
        out = obig[offset:offset + rows * n].reshape(rows, n, 1)
        plan = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dct=True, dct_type=4)
        mf.fft(out, x, plan=plan)
        torch.cuda.synchronize()
        assert torch.isnan(obig[:offset]).all() and torch.isnan(obig[offset + rows * n:]).all()
        assert _rel(out[..., 0].cpu().numpy(), ref_dct4(xn, None, inverse)) <= TOL[dtype]
    assert torch.equal(mf.dct(big[offset:offset + n], type=4), mf.dct(big[offset:offset + n].clone(), type=4))


def test_wrappers_shapes_and_dtypes():
    x = torch.randn(4, 6, 64, device=DEV)
    X = mf.dct(x, type=4)
    assert X.shape == x.shape and X.dtype == torch.float32
    xn = x.reshape(24, 64).cpu().numpy()
    assert _rel(X.reshape(24, 64).cpu().numpy(), ref_dct4(xn)) <= REL_L2_TOL_F32
    Xd = mf.dct(x, type=4, out_dtype=torch.float64)  # (converted first: the DCT-IV reads the plan's own float type)
    assert Xd.dtype == torch.float64 and _rel(Xd.reshape(24, 64).cpu().numpy(), ref_dct4(xn)) <= REL_L2_TOL_F64
    xi = torch.randint(-100, 100, (5, 32), dtype=torch.int16, device=DEV)
    Xi = mf.dct(xi, type=4)
    assert Xi.dtype == torch.float64 and _rel(Xi.cpu().numpy(), ref_dct4(xi.cpu().numpy())) <= REL_L2_TOL_F64
    v = torch.randn(64, device=DEV, dtype=torch.float64)  # a 1-D tensor is a batch of 1
    V = mf.idct(v, type=4, norm="ortho")
    assert V.shape == (64,) and _rel(V.cpu().numpy()[None], ref_dct4(v.cpu().numpy()[None], "ortho", True)) <= REL_L2_TOL_F64
    base = torch.randn(6, 5, 128, device=DEV)
    view = base.transpose(0, 1)[:, ::2, :]
    assert not view.is_contiguous() and torch.equal(mf.dct(view, type=4), mf.dct(view.contiguous(), type=4))
    with pytest.raises(mf.MifftError) as e:
        mf.dctn(x, type=4)
    assert e.value.status == -15
    # type 2 is what it was
    assert mf.plan_fft(torch.float32, torch.float32, (3, 64, 1), (3, 64, 1), dct=True).kernel_name(0).find("_dct2_") > 0


def test_user_radices_follow_the_tag():
    shape = (5, 1024, 1)
    x = torch.randn(shape, device=DEV)
    out = torch.empty_like(x)
    plan = mf.plan_fft(torch.float32, torch.float32, shape, shape, dct=True, dct_type=4, bases=[[8, 4, 2]])
    assert int(np.prod(plan.stages(0))) == 512 and set(plan.stages(0)) <= {8, 4, 2}
    mf.fft(out, x, plan=plan)
    torch.cuda.synchronize()
    assert _rel(out[..., 0].cpu().numpy(), ref_dct4(x[..., 0].cpu().numpy())) <= REL_L2_TOL_F32


def test_refused_without_runtime_specialisation():
    """MIFFT_JIT=0 (a fresh process: the switch is read once per process): the DCT-IV kernels are compiled at run time only"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "import hackathon_fft_amd as mf\n"
            "try:\n"
            "    mf.dct(torch.zeros(3, 64, device='cuda:0'), type=4)\n"
            "    print('planned')\n"
            "except mf.MifftError as e:\n"
            "    print(e.status, e)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("-15 ") and "MIFFT_JIT=0" in r.stdout and "run time" in r.stdout, r.stdout
