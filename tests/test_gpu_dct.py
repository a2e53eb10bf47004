"""DCT-II and its inverse on the MI355X (MIFFT_FLAG_DCT): the packed real-row kernels with TileCfg::DCT against an fp64 numpy
reference that does not go Makhoul's route -- the 4n-point complex FFT of the zero-interleaved even extension."""
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
NORMS = [None, "ortho"]


def _rel(got, ref):
    """max over the rows of ||got - ref|| / ||ref|| (real arrays, leading axis = batch)"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.float64).reshape(b, -1)
    r = np.asarray(ref, dtype=np.float64).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _ortho_scale(n):
    s = np.full(n, np.sqrt(1.0 / (2 * n)))
    s[0] = np.sqrt(1.0 / (4 * n))
    return s


def ref_dct(x, norm=None):
    """scipy.fft.dct(x, 2, norm=norm) of the rows of x in fp64: y[2j+1] = y[4n-2j-1] = x[j], X = Re(fft(y))[:n]"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    y = np.zeros(x.shape[:-1] + (4 * n,))
    y[..., 1:2 * n:2] = x
    y[..., 4 * n - 1:2 * n:-2] = x
    X = np.fft.fft(y, axis=-1).real[..., :n]
    return X * _ortho_scale(n) if norm == "ortho" else X


def ref_idct(X, norm=None):
    """scipy.fft.idct(X, 2, norm=norm) in fp64: Z[0] = X[0], Z[k] = 2 X[k], zeros to 4n; x[j] = Re(4n ifft(Z))[2j+1] / 2n"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[-1]
    if norm == "ortho":
        X = X / _ortho_scale(n)
    Z = np.zeros(X.shape[:-1] + (4 * n,))
    Z[..., :n] = 2 * X
    Z[..., 0] = X[..., 0]
    z = 4 * n * np.fft.ifft(Z, axis=-1)
    return z.real[..., 1:2 * n:2] / (2 * n)


def test_the_reference_is_the_cosine_sum():
    """the two references against the definition at small n (where the cosine matrix is still accurate)"""
    rng = np.random.default_rng(1)
    for n in (8, 30, 64):
        x = rng.standard_normal((3, n))
        j = np.arange(n)
        C = 2 * np.cos(np.pi * j[:, None] * (2 * j[None, :] + 1) / (2 * n))  # [k, j]
        assert np.abs(ref_dct(x) - x @ C.T).max() < 1e-12
        assert np.abs(ref_idct(x @ C.T) - x).max() < 1e-12
        Co = C * _ortho_scale(n)[:, None]
        assert np.abs(Co @ Co.T - np.eye(n)).max() < 1e-13
        assert np.abs(ref_dct(x, "ortho") - x @ Co.T).max() < 1e-12
        assert np.abs(ref_idct(x, "ortho") - x @ Co).max() < 1e-12


def _run(x_np, dtype, *, inverse, norm=None, in_dtype=None, first=None, count=None):
    """through a Plan: NaN-prefilled output, x checked unchanged; returns (fp64 result, plan)"""
    in_dtype = in_dtype or dtype
    xd = torch.from_numpy(np.ascontiguousarray(x_np)).to(DEV).to(in_dtype).unsqueeze(-1).contiguous()
    keep = xd.clone()
    shape = tuple(xd.shape)
    out = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(in_dtype, dtype, shape, shape, inverse=inverse, dct=True, norm=norm)
    if first is None:
        mf.fft(out, xd, plan=plan)
    else:
        mf.fft(out, xd, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    return out.cpu().numpy()[..., 0].astype(np.float64), plan


# (batch, n), fp64 too? -- batches leave ragged row tiles
SHAPES = [((37, 8), True),      # N = 4
          ((29, 16), True),
          ((23, 30), True),     # N = 15: odd N, no self-paired bin
          ((21, 480), True),
          ((19, 1024), True),   # the precompiled instance
          ((13, 1080), True),
          ((11, 686), True),    # N = 343, hipRTC
          ((3, 8192), True),    # the longest fp64 power of two
          ((2, 16384), False)]  # the longest row
CASES = [(s, torch.float32) for s, _ in SHAPES] + [(s, torch.float64) for s, f64 in SHAPES if f64]


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_forward_matches_the_reference(shape, dtype, norm):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(NP[dtype])
    got, plan = _run(x, dtype, inverse=False, norm=norm)
    assert not np.isnan(got).any()
    err = _rel(got, ref_dct(x, norm))
    print(f"dct {shape} {dtype} norm={norm}: rel L2 {err:.3e} {plan.kernel_name(0)}")
    assert err <= TOL[dtype], (shape, err, plan.kernel_name(0))


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_inverse_matches_the_reference(shape, dtype, norm):
    rng = np.random.default_rng(sum(shape) + 1)
    X = rng.standard_normal(shape).astype(NP[dtype])
    got, plan = _run(X, dtype, inverse=True, norm=norm)
    assert not np.isnan(got).any()
    err = _rel(got, ref_idct(X, norm))
    print(f"idct {shape} {dtype} norm={norm}: rel L2 {err:.3e} {plan.kernel_name(0)}")
    assert err <= TOL[dtype], (shape, err, plan.kernel_name(0))


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
@pytest.mark.parametrize("n", [30, 1024])
def test_structured_input_bin_by_bin(n, dtype):
    """unit impulses and a constant row: an index slip in the four-way store would hide inside an L2 norm.  The mirror for the
    four-way load of the inverse: unit coefficients, whose rows have norm sqrt(2n) / 2n (bin 0: sqrt(n) / 2n) where the forward's
    have sqrt(2n), so the forward's absolute tolerance TOL * sqrt(n) scales by 1 / 2n."""
    tol = TOL[dtype]
    odd = 2 * (n // 6) + 1
    x = np.zeros((4, n), dtype=NP[dtype])
    x[0, 0] = x[1, n - 1] = x[2, odd] = 1.0
    c = 0.75
    x[3, :] = c
    got, _ = _run(x, dtype, inverse=False)
    assert not np.isnan(got).any()
    k = np.arange(n)
    for row, j in ((0, 0), (1, n - 1), (2, odd)):
        want = 2 * np.cos(np.pi * k * (2 * j + 1) / (2 * n))
        assert np.abs(got[row] - want).max() <= tol * np.sqrt(n), (row, j, np.abs(got[row] - want).argmax())
    assert abs(got[3, 0] - 2 * n * c) <= tol * 2 * n * c
    assert np.abs(got[3, 1:]).max() <= tol * abs(2 * n * c), np.abs(got[3, 1:]).argmax() + 1
    # the inverse of unit impulses in the coefficients: bin 0, the last bin and an odd one
    back, _ = _run(x[:3], dtype, inverse=True)
    j = np.arange(n)
    for row, kk in ((0, 0), (1, n - 1), (2, odd)):
        want = (1.0 if kk == 0 else 2 * np.cos(np.pi * kk * (2 * j + 1) / (2 * n))) / (2 * n) * np.ones(n)
        assert np.abs(back[row] - want).max() <= tol * np.sqrt(n) / (2 * n), (row, kk)


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape", [(7, 30), (5, 480), (4, 1024)], ids=str)
def test_round_trips(shape, dtype, norm):
    tol = TOL[dtype]
    x = torch.randn(shape, dtype=dtype, device=DEV)
    X = mf.dct(x, norm=norm)
    assert X.shape == x.shape and X.dtype == dtype
    xn, Xn = x.cpu().numpy(), X.cpu().numpy()
    assert _rel(mf.idct(X, norm=norm).cpu().numpy(), xn) <= tol
    assert _rel(mf.dct(mf.idct(x, norm=norm), norm=norm).cpu().numpy(), xn) <= tol
    if norm == "ortho":  # Parseval
        nx, nX = np.linalg.norm(xn.astype(np.float64), axis=1), np.linalg.norm(Xn.astype(np.float64), axis=1)
        assert (np.abs(nX - nx) <= TOL[dtype] * nx).all()


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.int16, torch.float16, torch.bfloat16], ids=str)
def test_narrow_forward_input_types_are_widened(in_dtype):
    shape = (9, 480)
    rng = np.random.default_rng(7)
    if in_dtype == torch.uint8:
        xt = torch.from_numpy(rng.integers(0, 256, size=shape).astype(np.uint8))
    elif in_dtype == torch.int16:
        xt = torch.from_numpy(rng.integers(-30000, 30000, size=shape).astype(np.int16))
    else:
        xt = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(in_dtype)
    wide = xt.to(torch.float64).numpy()
    src = xt.numpy() if in_dtype in (torch.uint8, torch.int16) else xt.float().numpy()  # (exact in float32)
    got, plan = _run(src, torch.float32, inverse=False, in_dtype=in_dtype)
    assert plan.in_dtype == in_dtype
    err = _rel(got, ref_dct(wide))
    assert err <= REL_L2_TOL_F32, err
    y = mf.dct(xt.to(DEV))  # the wrapper widens an input that is neither float32 nor float64 to float64
    assert y.dtype == torch.float64
    assert _rel(y.cpu().numpy(), ref_dct(wide)) <= REL_L2_TOL_F64


def test_wrappers_shapes_and_dtypes():
    x = torch.randn(4, 6, 64, device=DEV)
    X = mf.dct(x)
    assert X.shape == x.shape and X.dtype == torch.float32
    assert _rel(X.reshape(24, 64).cpu().numpy(), ref_dct(x.reshape(24, 64).cpu().numpy())) <= REL_L2_TOL_F32
    Xd = mf.dct(x, out_dtype=torch.float64)
    assert Xd.dtype == torch.float64 and _rel(Xd.reshape(24, 64).cpu().numpy(), ref_dct(x.reshape(24, 64).cpu().numpy())) <= REL_L2_TOL_F64
    y = mf.idct(X, norm="ortho", out_dtype=torch.float64)
    assert y.shape == x.shape and y.dtype == torch.float64
    assert _rel(y.reshape(24, 64).cpu().numpy(), ref_idct(X.reshape(24, 64).cpu().numpy(), "ortho")) <= REL_L2_TOL_F64
    v = torch.randn(64, device=DEV, dtype=torch.float64)  # a 1-D tensor is a batch of 1
    V = mf.dct(v, norm="ortho")
    assert V.shape == (64,) and V.dtype == torch.float64
    assert _rel(V.cpu().numpy()[None], ref_dct(v.cpu().numpy()[None], "ortho")) <= REL_L2_TOL_F64
    assert mf.dct(x.unsqueeze(-1), dim=2).shape == (4, 6, 64, 1)  # trailing dims of size 1 do not count
    with pytest.raises(mf.MifftError) as e:
        mf.dct(x, dim=1)
    assert e.value.status == -15


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_base_pointer_aligned_to_one_element_only(offset, dtype):
    """contiguous slices at a storage offset of 1 .. 3 elements, on both sides: the kernels' four-real accesses (an even n / 2)
    are then aligned to one element only, the contract of include/mifft.h"""
    n, rows = 64, 5
    big = torch.randn(offset + rows * n, dtype=dtype, device=DEV)
    x = big[offset:].reshape(rows, n, 1)
    assert x.is_contiguous() and x.data_ptr() % (4 * x.element_size()) != 0
    xn = x[..., 0].cpu().numpy()
    for inverse, ref in ((False, ref_dct), (True, ref_idct)):
        obig = torch.full((offset + rows * n,), float("nan"), dtype=dtype, device=DEV)
        out = obig[offset:].reshape(rows, n, 1)
        plan = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dct=True)
        mf.fft(out, x, plan=plan)
        torch.cuda.synchronize()
        assert torch.isnan(obig[:offset]).all()
        assert _rel(out[..., 0].cpu().numpy(), ref(xn)) <= TOL[dtype]
    assert torch.equal(mf.dct(big[offset:offset + n]), mf.dct(big[offset:offset + n].clone()))


def test_a_non_contiguous_view_equals_its_contiguous_copy():
    base = torch.randn(6, 5, 128, device=DEV)
    view = base.transpose(0, 1)[:, ::2, :]
    assert not view.is_contiguous()
    assert torch.equal(mf.dct(view), mf.dct(view.contiguous()))
    assert torch.equal(mf.idct(view, norm="ortho"), mf.idct(view.contiguous(), norm="ortho"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [1024, 480])
def test_introspection(n, dtype):
    esz = 4 if dtype == torch.float32 else 8
    shape = (5, n, 1)
    for inverse, tag in ((False, "dct2"), (True, "dct3")):
        plan = mf.plan_fft(dtype, dtype, shape, shape, inverse=inverse, dct=True)
        name = plan.kernel_name(0)
        assert name.startswith(f"rows{n}_" + ("f64_" if dtype == torch.float64 else "") + tag + "_"), name
        assert name.endswith("_jit") == (n != 1024), name
        assert plan.num_launches == 1 and plan.scratch_bytes == 0
        assert plan.in_bytes == plan.out_bytes == 5 * n * esz
        stages = plan.stages(0)
        assert int(np.prod(stages)) == n // 2, stages  # the stages of the packed n / 2-point transform


def test_1024_points_plan_and_match_without_runtime_specialisation():
    """MIFFT_JIT=0 (a fresh process, with its own time limit): 1024 points run on the precompiled instances, fp32 and fp64,
    both directions, and agree with this process's reference; 1000 points are refused with the reason."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, torch\n"
            "import hackathon_fft_amd as mf\n"
            "from test_gpu_dct import ref_dct, ref_idct, _rel, _run\n"
            "for dtype, tol in ((torch.float32, %r), (torch.float64, %r)):\n"
            "    x = np.random.default_rng(3).standard_normal((6, 1024))\n"
            "    for inv, ref in ((False, ref_dct), (True, ref_idct)):\n"
            "        xq = x.astype(np.float32 if dtype == torch.float32 else np.float64)\n"
            "        got, plan = _run(xq, dtype, inverse=inv)\n"
            "        err = _rel(got, ref(xq))\n"
            "        print(plan.kernel_name(0), err, err <= tol)\n"
            "try:\n"
            "    mf.dct(torch.zeros(2, 1000, device='cuda:0'))\n"
            "    print('planned')\n"
            "except mf.MifftError as e:\n"
            "    print('refused', e.status, 'MIFFT_JIT=0' in str(e))\n" % (ROOT, os.path.join(ROOT, "tests"), REL_L2_TOL_F32, REL_L2_TOL_F64))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5, r.stdout
    for ln, tag in zip(lines[:4], ("_dct2_", "_dct3_", "_f64_dct2_", "_f64_dct3_")):
        name, err, ok = ln.split()
        assert tag in name and not name.endswith("_jit") and ok == "True", ln
    assert lines[4] == "refused -15 True", lines[4]
