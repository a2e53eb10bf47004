"""DST-II / its inverse and DST-IV of real rows on the MI355X (MIFFT_DST_TAG / MIFFT_DST_TYPE4_TAG): the TileCfg::DST kernels
against the fp64 numpy references of test_dst_host.py -- the sine matrices up to 1080 points, the cosine route beyond (both
checked against the explicit sums there)."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_dst_host import dst2_matrix, dst4_matrix, ref_dst2, ref_dst4
from test_gpu_dct import ref_dct

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]
REF = {2: ref_dst2, 4: ref_dst4}


def _rel(got, ref):
    """max over the rows of ||got - ref|| / ||ref|| (real arrays, leading axis = batch)"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.float64).reshape(b, -1)
    r = np.asarray(ref, dtype=np.float64).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _run(x_np, dtype, *, type, inverse, norm=None, in_dtype=None, first=None, count=None, dst=True):
    """through a Plan: NaN-prefilled output, x checked unchanged; returns (fp64 result, plan)"""
    in_dtype = in_dtype or dtype
    xd = torch.from_numpy(np.array(x_np)).to(DEV).to(in_dtype).unsqueeze(-1).contiguous()
    keep = xd.clone()
    shape = tuple(xd.shape)
    out = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(in_dtype, dtype, shape, shape, inverse=inverse, dct=True, dst=dst, dct_type=type, norm=norm)
    if first is None:
        mf.fft(out, xd, plan=plan)
    else:
        mf.fft(out, xd, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    return out.cpu().numpy()[..., 0].astype(np.float64), plan


def _kernel_word(type, inverse):
    return "dst4" if type == 4 else "dst3" if inverse else "dst2"


# (batch, n), fp64 too? -- odd batches leave ragged row tiles
SHAPES = [((37, 8), True),      # N = 4
          ((29, 16), True),
          ((23, 30), True),     # N = 15: no quads; the DCT-IV tile's middle work item is its own partner
          ((21, 480), True),
          ((19, 1024), True),
          ((11, 686), True),    # N = 343
          ((3, 8192), True),    # the longest fp64 power of two
          ((2, 16384), False)]  # the longest row
CASES = [(s, torch.float32) for s, _ in SHAPES] + [(s, torch.float64) for s, f64 in SHAPES if f64]
_INPUTS = {}


def _input(shape, dtype):
    """one input per (shape, dtype), and its references per (type, norm, inverse): computed once, left unchanged"""
    key = (shape, dtype)
    if key not in _INPUTS:
        x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(NP[dtype])
        x.setflags(write=False)
        _INPUTS[key] = (x, {})
    return _INPUTS[key]


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("inverse", [False, True], ids=["dst", "idst"])
@pytest.mark.parametrize("type", [2, 4])
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_both_directions_match_the_reference(shape, dtype, type, inverse, norm):
    x, refs = _input(shape, dtype)
    if (type, norm, inverse) not in refs:
        refs[(type, norm, inverse)] = REF[type](x, norm, inverse)
    got, plan = _run(x, dtype, type=type, inverse=inverse, norm=norm)
    assert not np.isnan(got).any()
    err = _rel(got, refs[(type, norm, inverse)])
    name = plan.kernel_name(0)
    print(f"{'idst' if inverse else 'dst'}{type} {shape} {dtype} norm={norm}: rel L2 {err:.3e} {name}")
    assert err <= TOL[dtype], (shape, err, name)
    n = shape[1]
    word = _kernel_word(type, inverse)
    assert name.startswith(f"rows{n}_" + ("f64_" if dtype == torch.float64 else "") + word + "_") and name.endswith("_jit"), name
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    assert int(np.prod(plan.stages(0))) == n // 2
    assert plan.dst and plan.dct and plan.dct_type == type
    esz = 4 if dtype == torch.float32 else 8
    assert plan.in_bytes == plan.out_bytes == shape[0] * n * esz


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("type", [2, 4])
@pytest.mark.parametrize("n", [30, 1024])
def test_structured_input_bin_by_bin(n, type, dtype):
    """unit impulses at both ends and both sides of the middle, and a constant row, every element compared: the DST-II store is
    a shift by one, so a slip moves a bin to its neighbour and hides inside an L2 norm.  A unit impulse has a transform of norm
    about sqrt(2n): the absolute tolerance is TOL sqrt(n)."""
    tol = TOL[dtype]
    where = [0, 1, n // 2 - 1, n // 2, n - 2, n - 1]
    x = np.zeros((len(where) + 1, n), dtype=NP[dtype])
    for row, j in enumerate(where):
        x[row, j] = 1.0
    c = 0.75
    x[-1, :] = c
    k = np.arange(n)

    def column(j):  # the transform of a unit impulse at j, from the definition
        if type == 2:
            return 2 * np.sin(np.pi * (k + 1) * (2 * j + 1) / (2 * n))
        return 2 * np.sin(np.pi * (2 * j + 1) * (2 * k + 1) / (4 * n))

    def row_of_inverse(kk):  # the inverse of a unit coefficient at kk, from the definition
        if type == 4:
            return column(kk) / (2 * n)
        j = k
        return (1.0 - 2.0 * (j & 1) if kk == n - 1 else 2 * np.sin(np.pi * (kk + 1) * (2 * j + 1) / (2 * n))) / (2 * n)

    got, _ = _run(x, dtype, type=type, inverse=False)
    assert not np.isnan(got).any()
    for row, j in enumerate(where):
        want = column(j)
        assert np.abs(got[row] - want).max() <= tol * np.sqrt(n), (row, j, int(np.abs(got[row] - want).argmax()))
    S = dst2_matrix(n).T if type == 2 else dst4_matrix(n)
    want = x[-1].astype(np.float64) @ S
    if type == 2:  # 2 c sum_j sin((k+1) (2j+1) h), h = pi / 2n: c (1 - cos(pi (k+1))) / sin((k+1) h) -- zero at the odd bins
        closed = c * (1 - np.cos(np.pi * (k + 1))) / np.sin(np.pi * (k + 1) / (2 * n))
    else:          # 2 c sum_j sin((2j+1) a), a = pi (2k+1) / 4n: c (1 - cos(2 n a)) / sin(a) = c / sin(a)
        closed = c / np.sin(np.pi * (2 * k + 1) / (4 * n))
    assert np.abs(want - closed).max() < 1e-9
    assert np.abs(got[-1] - closed).max() <= tol * np.abs(closed).max(), int(np.abs(got[-1] - closed).argmax())
    back, _ = _run(x[:-1], dtype, type=type, inverse=True)
    for row, kk in enumerate(where):
        want = row_of_inverse(kk)
        assert np.abs(back[row] - want).max() <= tol * np.sqrt(n) / (2 * n), (row, kk, int(np.abs(back[row] - want).argmax()))


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape", [(7, 30), (5, 480), (4, 1024)], ids=str)
def test_round_trips(shape, dtype, norm):
    tol = TOL[dtype]
    x = torch.randn(shape, dtype=dtype, device=DEV)
    xn = x.cpu().numpy()
    for t in (2, 4):
        X = mf.dst(x, type=t, norm=norm)
        assert X.shape == x.shape and X.dtype == dtype
        assert _rel(X.cpu().numpy(), REF[t](xn, norm)) <= tol
        assert _rel(mf.idst(X, type=t, norm=norm).cpu().numpy(), xn) <= tol
        assert _rel(mf.dst(mf.idst(x, type=t, norm=norm), type=t, norm=norm).cpu().numpy(), xn) <= tol
        if norm == "ortho":  # Parseval
            nx, nX = np.linalg.norm(xn.astype(np.float64), axis=1), np.linalg.norm(X.cpu().numpy().astype(np.float64), axis=1)
            assert (np.abs(nX - nx) <= tol * nx).all()
    X4 = mf.dst(x, type=4, norm="ortho")  # the orthonormal DST-IV: an involution, both directions the same kernel and scale
    assert _rel(mf.dst(X4, type=4, norm="ortho").cpu().numpy(), xn) <= tol
    assert torch.equal(mf.idst(x, type=4, norm="ortho"), X4)


def test_forward_type_2_widens_an_int16_input():
    xi = torch.randint(-3000, 3000, (9, 96), dtype=torch.int16, device=DEV)
    xf = xi.cpu().numpy().astype(np.float64)
    for dtype in (torch.float32, torch.float64):
        got, plan = _run(xi.cpu().numpy(), dtype, type=2, inverse=False, in_dtype=torch.int16)
        assert plan.kernel_name(0).startswith("rows96_" + ("f64_" if dtype == torch.float64 else "") + "dst2_"), plan.kernel_name(0)
        assert "_i16" in plan.kernel_name(0)
        assert _rel(got, ref_dst2(xf)) <= TOL[dtype]
        same, _ = _run(xf, dtype, type=2, inverse=False)  # the transform of its float conversion (exact in both types)
        assert _rel(got, same) <= TOL[dtype]
    X = mf.dst(xi)
    assert X.dtype == torch.float64 and _rel(X.cpu().numpy(), ref_dst2(xf)) <= REL_L2_TOL_F64
    X4 = mf.dst(xi, type=4)  # (converted first: the DST-IV reads the plan's own float type)
    assert X4.dtype == torch.float64 and _rel(X4.cpu().numpy(), ref_dst4(xf)) <= REL_L2_TOL_F64


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("type", [2, 4])
@pytest.mark.parametrize("n", [30, 1024])
def test_two_slabs_equal_the_whole_batch(n, type, inverse):
    rng = np.random.default_rng(n + type)
    x = rng.standard_normal((11, n)).astype(np.float32)
    whole, _ = _run(x, torch.float32, type=type, inverse=inverse)
    lo, _ = _run(x, torch.float32, type=type, inverse=inverse, first=0, count=4)
    hi, _ = _run(x, torch.float32, type=type, inverse=inverse, first=4, count=7)
    assert np.array_equal(lo[:4], whole[:4]) and np.isnan(lo[4:]).all()
    assert np.array_equal(hi[4:], whole[4:]) and np.isnan(hi[:4]).all()


@pytest.mark.parametrize("inverse", [False, True])
def test_a_dct_plan_of_the_same_shape_is_still_a_dct_plan(inverse):
    """the kernel cache and the plan cache key on the sine bit: after DST plans of a shape, the cosine plans of that shape
    report cosine kernels and compute the cosine transforms, and the other way round"""
    from test_dct4_host import ref_dct4
    from test_gpu_dct import ref_idct
    shape = (6, 256)
    x = np.random.default_rng(256).standard_normal(shape).astype(np.float32)
    for t in (2, 4):
        s, ps = _run(x, torch.float32, type=t, inverse=inverse)
        c, pc = _run(x, torch.float32, type=t, inverse=inverse, dst=False)
        s2, ps2 = _run(x, torch.float32, type=t, inverse=inverse)
        word = _kernel_word(t, inverse)
        assert f"_{word}_" in ps.kernel_name(0) and f"_{word}_" in ps2.kernel_name(0), ps.kernel_name(0)
        assert f"_{word.replace('dst', 'dct')}_" in pc.kernel_name(0) and "dst" not in pc.kernel_name(0), pc.kernel_name(0)
        assert pc.dst is False and ps.dst is True
        want_c = ref_dct4(x, None, inverse) if t == 4 else (ref_idct(x) if inverse else ref_dct(x))
        assert _rel(c, want_c) <= REL_L2_TOL_F32
        assert _rel(s, REF[t](x, None, inverse)) <= REL_L2_TOL_F32 and np.array_equal(s, s2)
    xd = torch.from_numpy(x).to(DEV)
    fs, fc = (mf.idst, mf.idct) if inverse else (mf.dst, mf.dct)
    for t in (2, 4):  # the wrappers' plan cache
        a, b, a2 = fs(xd, type=t), fc(xd, type=t), fs(xd, type=t)
        assert torch.equal(a, a2) and not torch.equal(a, b)
        want_c = ref_dct4(x, None, inverse) if t == 4 else (ref_idct(x) if inverse else ref_dct(x))
        assert _rel(b.cpu().numpy(), want_c) <= REL_L2_TOL_F32
        assert _rel(a.cpu().numpy(), REF[t](x, None, inverse)) <= REL_L2_TOL_F32


def test_wrappers_shapes_dtypes_and_user_radices():
    x = torch.randn(4, 6, 64, device=DEV)
    xn = x.reshape(24, 64).cpu().numpy()
    for t in (2, 4):
        X = mf.dst(x, type=t)
        assert X.shape == x.shape and X.dtype == torch.float32
        assert _rel(X.reshape(24, 64).cpu().numpy(), REF[t](xn)) <= REL_L2_TOL_F32
        Xd = mf.dst(x, type=t, out_dtype=torch.float64)
        assert Xd.dtype == torch.float64 and _rel(Xd.reshape(24, 64).cpu().numpy(), REF[t](xn)) <= REL_L2_TOL_F64
    v = torch.randn(64, device=DEV, dtype=torch.float64)  # a 1-D tensor is a batch of 1
    V = mf.idst(v, norm="ortho")
    assert V.shape == (64,) and _rel(V.cpu().numpy()[None], ref_dst2(v.cpu().numpy()[None], "ortho", True)) <= REL_L2_TOL_F64
    shape = (5, 1024, 1)
    xs = torch.randn(shape, device=DEV)
    for t in (2, 4):  # radices behind the tag
        out = torch.empty_like(xs)
        plan = mf.plan_fft(torch.float32, torch.float32, shape, shape, dct=True, dst=True, dct_type=t, bases=[[8, 4, 2]])
        assert int(np.prod(plan.stages(0))) == 512 and set(plan.stages(0)) <= {8, 4, 2}
        mf.fft(out, xs, plan=plan)
        torch.cuda.synchronize()
        assert _rel(out[..., 0].cpu().numpy(), REF[t](xs[..., 0].cpu().numpy())) <= REL_L2_TOL_F32
    for t in (1, 3):
        with pytest.raises(mf.MifftError) as e:
            mf.dst(x, type=t)
        assert e.value.status == -15
