"""N-D DST-II and its inverse on the MI355X (MIFFT_DST_TAG on a MIFFT_FLAG_DCT_ND plan): the paired-column tiles and the packed
rows with TileCfg::DST against the separable fp64 reference of test_dst_host.py (the sine matrix along every transformed axis)."""
import re

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_dst_host import ref_dstn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]
DTYPES = [torch.float32, torch.float64]

_CACHE = {}


def _rel(got, ref):
    """max over the batch entries of ||got - ref|| / ||ref||"""
    b = got.shape[0]
    g = np.asarray(got, dtype=np.float64).reshape(b, -1)
    r = np.asarray(ref, dtype=np.float64).reshape(b, -1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _ref(shape, dtype, dim, inverse, norm):
    """one input per (shape, dtype) and one reference per (dim, inverse, norm): computed once, left unchanged"""
    if (shape, dtype) not in _CACHE:
        x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(NP[dtype])
        x.setflags(write=False)
        _CACHE[(shape, dtype)] = (x, {})
    x, refs = _CACHE[(shape, dtype)]
    k = (dim, inverse, norm)
    if k not in refs:
        refs[k] = ref_dstn(x, dim, inverse, norm)
    return x, refs[k]


def _run(x_np, dtype, dim, *, inverse, norm=None, dst=True):
    """through a Plan over the reduced (batch, e0.., 1) layout of x_np: NaN-prefilled output, x checked unchanged; returns
    (fp64 result in the shape of x_np, plan, the layout positions transformed)"""
    layout, axes = mf.reduce_dims(x_np.shape, dim)
    shape = tuple(layout) + (1,)
    xd = torch.from_numpy(np.array(x_np)).to(DEV).to(dtype).reshape(shape).contiguous()
    keep = xd.clone()
    out = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(dtype, dtype, shape, shape, inverse=inverse, dctn=True, dst=dst, norm=norm,
                       axes=None if len(axes) == len(layout) - 1 else axes)
    mf.fft(out, xd, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    return out.cpu().numpy().astype(np.float64).reshape(x_np.shape), plan, tuple(axes)


# (shape, dim): dim as the wrappers take it, None = every dim but the first
CASES = [((3, 6, 8), None),             # the shortest column next to the shortest row
         ((2, 5, 9, 8), None),          # odd column lengths
         ((2, 30, 16), None),
         ((2, 16, 50), None),           # 25 column pairs: a ragged column tile
         ((4, 12, 6), (1,)),            # the column pass only, stride 6, the last dim kept
         ((2, 4, 8, 4, 8), (2, 4)),     # 8 x 8 blocks through a kept dim
         ((1, 64, 48), None)]


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("inverse", [False, True], ids=["dstn", "idstn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape,dim", CASES, ids=str)
def test_matches_the_separable_reference(shape, dim, dtype, inverse, norm):
    dims = tuple(range(1, len(shape))) if dim is None else dim
    x, ref = _ref(shape, dtype, dims, inverse, norm)
    fn = mf.idstn if inverse else mf.dstn
    xd = torch.from_numpy(x.copy()).to(DEV)
    keep = xd.clone()
    got = fn(xd, norm=norm, dim=dim)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    assert got.shape == xd.shape and got.dtype == dtype
    err = _rel(got.cpu().numpy(), ref)
    # ... and the same through a plan with NaN behind it: one launch per transformed dim, every kernel a sine kernel
    got2, plan, axes = _run(x, dtype, dims, inverse=inverse, norm=norm)
    names = [plan.kernel_name(d) for d in range(plan.ndim)]
    print(f"{fn.__name__} {shape} dim={dim} {dtype} norm={norm}: rel L2 {err:.3e} {names}")
    assert err <= TOL[dtype], (shape, dim, err, names)
    assert not np.isnan(got2).any() and _rel(got2, ref) <= TOL[dtype]
    assert plan.dst and plan.dctn
    assert plan.num_launches == len(dims) and plan.scratch_bytes == 0
    word = "dst3" if inverse else "dst2"
    f64 = "f64_" if dtype == torch.float64 else ""
    for d in range(plan.ndim):
        n = plan.out_shape[1 + d]
        if d + 1 not in axes:
            assert names[d] == "none", names
        elif d == plan.ndim - 1:
            assert re.fullmatch(rf"rows{n}_{f64}{word}_[0-9x]+(_ntl)?_jit", names[d]), names
            assert int(np.prod(plan.stages(d))) == n // 2
        else:
            assert re.fullmatch(rf"cols{n}_{f64}{word}_[0-9x]+_jit", names[d]), names
            assert int(np.prod(plan.stages(d))) == n


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_row_impulses_bin_by_bin(dtype):
    """the (2, 30, 16) case along dim 1: every real column carries a unit-sized impulse at row 0, 1, n - 2 or n - 1, its pair
    partner at another of them with another amplitude.  A slip in the reversing store (or the reversed combining load of the
    inverse) moves a bin to its neighbour, leakage between the columns of a pair mixes amplitudes: both hide in an L2 norm.
    Every element against the sine formula, absolute tolerance TOL * sqrt(n) (inverse: scaled by 1 / 2n)."""
    n, tol = 30, TOL[dtype]
    where = [0, 1, n - 2, n - 1]
    k = np.arange(n)
    x = np.zeros((2, n, 16), dtype=NP[dtype])
    want_f, want_i = np.zeros((2, n, 16)), np.zeros((2, n, 16))

    def fwd(j):
        return 2 * np.sin(np.pi * (k + 1) * (2 * j + 1) / (2 * n))

    def inv(kk):
        return (1.0 - 2.0 * (k & 1) if kk == n - 1 else 2 * np.sin(np.pi * (kk + 1) * (2 * k + 1) / (2 * n))) / (2 * n)

    for b in range(2):
        for c in range(16):
            r, amp = where[(c + c // 4 + b) % 4], 1.0 - c / 32.0  # (the two columns of a pair: different rows and amplitudes)
            x[b, r, c] = amp
            want_f[b, :, c], want_i[b, :, c] = amp * fwd(r), amp * inv(r)
    got, plan, _ = _run(x, dtype, (1,), inverse=False)
    assert not np.isnan(got).any()
    assert plan.kernel_name(0).startswith("cols30_") and "_dst2_" in plan.kernel_name(0), plan.kernel_name(0)
    d = np.abs(got - want_f)
    assert d.max() <= tol * np.sqrt(n), ("forward", np.unravel_index(d.argmax(), d.shape), d.max())
    back, plan, _ = _run(x, dtype, (1,), inverse=True)
    assert not np.isnan(back).any() and "_dst3_" in plan.kernel_name(0)
    d = np.abs(back - want_i)
    assert d.max() <= tol * np.sqrt(n) / (2 * n), ("inverse", np.unravel_index(d.argmax(), d.shape), d.max())
    # both dims: an impulse at (r, q) becomes the outer product of the two sine vectors (norm 2 sqrt(n m): TOL sqrt(n m))
    m = 16
    kq = np.arange(m)
    y = np.zeros((2, n, m), dtype=NP[dtype])
    want = np.zeros((2, n, m))
    for b, (r, q) in enumerate(((1, m - 1), (n - 1, 0))):
        y[b, r, q] = 1.0
        want[b] = np.outer(fwd(r), 2 * np.sin(np.pi * (kq + 1) * (2 * q + 1) / (2 * m)))
    got, _, _ = _run(y, dtype, (1, 2), inverse=False)
    d = np.abs(got - want)
    assert d.max() <= tol * np.sqrt(n * m), ("2-D", np.unravel_index(d.argmax(), d.shape), d.max())


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(2, 30, 16), (2, 5, 9, 8)], ids=str)
def test_round_trips(shape, dtype, norm):
    tol = TOL[dtype]
    x = torch.randn(shape, dtype=dtype, device=DEV)
    X = mf.dstn(x, norm=norm)
    assert X.shape == x.shape and X.dtype == dtype
    xn, Xn = x.cpu().numpy(), X.cpu().numpy()
    assert _rel(mf.idstn(X, norm=norm).cpu().numpy(), xn) <= tol
    assert _rel(mf.dstn(mf.idstn(x, norm=norm), norm=norm).cpu().numpy(), xn) <= tol
    if norm == "ortho":  # Parseval
        b = shape[0]
        nx = np.linalg.norm(xn.astype(np.float64).reshape(b, -1), axis=1)
        nX = np.linalg.norm(Xn.astype(np.float64).reshape(b, -1), axis=1)
        assert (np.abs(nX - nx) <= tol * nx).all()


def test_a_dctn_plan_of_the_same_shape_is_still_a_dctn_plan():
    shape = (2, 30, 16)
    x = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    s, ps, _ = _run(x, torch.float32, (1, 2), inverse=False)
    c, pc, _ = _run(x, torch.float32, (1, 2), inverse=False, dst=False)
    assert "_dst2_" in ps.kernel_name(0) and "_dst2_" in ps.kernel_name(1)
    assert "_dct2_" in pc.kernel_name(0) and "_dct2_" in pc.kernel_name(1) and pc.dst is False
    assert _rel(s, ref_dstn(x, (1, 2))) <= REL_L2_TOL_F32
    xd = torch.from_numpy(x).to(DEV)
    a, b, a2 = mf.dstn(xd), mf.dctn(xd), mf.dstn(xd)  # the wrappers' plan cache
    assert torch.equal(a, a2) and np.array_equal(a.cpu().numpy().astype(np.float64), s)
    assert np.array_equal(b.cpu().numpy().astype(np.float64), c) and not torch.equal(a, b)


@pytest.mark.parametrize("fn,cos", [(mf.dstn, mf.dctn), (mf.idstn, mf.idctn)], ids=["dstn", "idstn"])
def test_strides_of_2_and_odd_strides_are_refused_as_dctn_refuses_them(fn, cos):
    for shape, word in (((3, 16, 2), "stride of 2"), ((3, 16, 5), "odd stride"), ((3, 16, 7, 3), "odd stride")):
        x = torch.zeros(shape, device=DEV)
        with pytest.raises(mf.MifftError) as e:
            fn(x, dim=1)
        with pytest.raises(mf.MifftError) as ec:
            cos(x, dim=1)
        assert e.value.status == ec.value.status == -15 and word in str(e.value), (shape, str(e.value))
        assert str(e.value) == str(ec.value)
    with pytest.raises(mf.MifftError) as e:
        fn(torch.zeros(3, 16, 64, device=DEV), type=4)
    assert e.value.status == -15


@pytest.mark.parametrize("inverse", [False, True], ids=["dstn", "idstn"])
def test_a_kept_first_dim_carries_the_tag_alone(inverse):
    """a plan made by hand whose dimension 0 is kept (the wrappers fold such a dim into the batch): its list holds the tag and
    nothing else, the transformed dim behind it takes its default radices or the user's"""
    shape = (3, 5, 64)
    x = np.random.default_rng(64).standard_normal(shape).astype(np.float32)
    ref = ref_dstn(x, (2,), inverse)
    xd = torch.from_numpy(x).to(DEV).unsqueeze(-1).contiguous()
    for bases in (None, [[], [8, 4]]):
        out = torch.full_like(xd, float("nan"))
        plan = mf.plan_fft(torch.float32, torch.float32, xd.shape, xd.shape, inverse=inverse, dctn=True, dst=True, axes=(2,),
                           bases=bases)
        mf.fft(out, xd, plan=plan)
        torch.cuda.synchronize()
        word = "dst3" if inverse else "dst2"
        assert plan.kernel_name(0) == "none" and f"rows64_{word}_" in plan.kernel_name(1), (plan.kernel_name(0), plan.kernel_name(1))
        assert plan.stages(0) == [] and int(np.prod(plan.stages(1))) == 32 and plan.num_launches == 1
        if bases is not None:
            assert set(plan.stages(1)) <= {8, 4}
        assert _rel(out[..., 0].cpu().numpy(), ref) <= REL_L2_TOL_F32
