"""N-D DCT-II and its inverse on the MI355X (MIFFT_FLAG_DCT_ND): the packed-row DCT kernel for a transformed last dim and
the paired-column tiles (TileCfg::DCT on a column configuration) for every other one, against the fp64 numpy reference of
test_gpu_dct.py applied along each transformed axis."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import ROOT, REL_L2_TOL_F32, REL_L2_TOL_F64
from test_gpu_dct import _rel, ref_dct, ref_idct

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]
DTYPES = [torch.float32, torch.float64]
FAR = 1 << 40  # a count at which no grid is clamped by the tile count

_REF_CACHE = {}


def ref_nd(x, axes, inverse=False, norm=None):
    """ref_dct / ref_idct of test_gpu_dct.py along every axis of `axes` (positions in x), in fp64"""
    y = np.asarray(x, dtype=np.float64)
    f = ref_idct if inverse else ref_dct
    for a in axes:
        y = np.moveaxis(f(np.moveaxis(y, a, -1), norm), -1, a)
    return y


def _input(shape, dtype, seed):
    """one input per (shape, dtype, seed) and its references, computed once and left unchanged"""
    key = (shape, dtype, seed)
    if key not in _REF_CACHE:
        x = np.random.default_rng(seed).standard_normal(shape).astype(NP[dtype])
        x.setflags(write=False)
        _REF_CACHE[key] = (x, {})
    return _REF_CACHE[key]


def _ref(shape, dtype, seed, axes, inverse, norm):
    x, refs = _input(shape, dtype, seed)
    k = (tuple(axes), inverse, norm)
    if k not in refs:
        refs[k] = ref_nd(x, axes, inverse, norm)
    return x, refs[k]


def _run(x_np, dtype, *, inverse, norm=None, axes=None, in_dtype=None, first=None, count=None):
    """through a Plan over the (batch, d0.., 1) layout of x_np: NaN-prefilled output, x checked unchanged; returns (fp64
    result, plan)"""
    in_dtype = in_dtype or dtype
    xd = torch.from_numpy(np.array(x_np)).to(DEV).to(in_dtype).unsqueeze(-1).contiguous()
    keep = xd.clone()
    shape = tuple(xd.shape)
    out = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    plan = mf.plan_fft(in_dtype, dtype, shape, shape, inverse=inverse, dctn=True, norm=norm, axes=axes)
    if first is None:
        mf.fft(out, xd, plan=plan)
    else:
        mf.fft(out, xd, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    return out.cpu().numpy()[..., 0].astype(np.float64), plan


# ---- parity ------------------------------------------------------------------------------------------------------------------

SHAPES = [(5, 8, 38),       # 19 paired columns: one ragged tile
          (3, 15, 64),      # odd column length
          (3, 30, 70),      # self-paired bin, ragged second tile
          (2, 64, 64),
          (2, 6, 15, 16),   # 3-D with two column passes
          (2, 480, 64),
          (1, 2, 8),        # the shortest columns
          (1, 3, 8)]


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("inverse", [False, True], ids=["dctn", "idctn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_matches_the_reference(shape, dtype, inverse, norm):
    axes = tuple(range(1, len(shape)))
    x, ref = _ref(shape, dtype, sum(shape), axes, inverse, norm)
    got, plan = _run(x, dtype, inverse=inverse, norm=norm)
    assert not np.isnan(got).any()
    err = _rel(got, ref)
    names = [plan.kernel_name(d) for d in range(plan.ndim)]
    print(f"{'idctn' if inverse else 'dctn'} {shape} {dtype} norm={norm}: rel L2 {err:.3e} {names}")
    assert err <= TOL[dtype], (shape, err, names)


# ---- subsets of the dims -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("inverse", [False, True], ids=["dctn", "idctn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape,dim", [((4, 30, 38), (1,)),            # the column pass first, out of place
                                       ((2, 16, 5, 32), (1, 3))],      # a kept dim between
                         ids=str)
def test_a_subset_of_the_dims(shape, dim, dtype, inverse, norm):
    x, ref = _ref(shape, dtype, 11 + sum(shape), dim, inverse, norm)
    fn = mf.idctn if inverse else mf.dctn
    xd = torch.from_numpy(x.copy()).to(DEV)
    keep = xd.clone()
    got = fn(xd, norm=norm, dim=dim)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "x was written"
    assert got.shape == xd.shape and got.dtype == dtype
    err = _rel(got.cpu().numpy(), ref)
    print(f"{fn.__name__} {shape} dim={dim} {dtype} norm={norm}: rel L2 {err:.3e}")
    assert err <= TOL[dtype], (shape, dim, err)
    # ... and the same through a plan with NaN behind it
    got2, plan = _run(x, dtype, inverse=inverse, norm=norm, axes=dim)
    assert not np.isnan(got2).any()
    assert plan.num_launches == len(dim)
    assert _rel(got2, ref) <= TOL[dtype]


@pytest.mark.parametrize("inverse", [False, True], ids=["dctn", "idctn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_8x8_blocks(dtype, inverse):
    B, H, W = 2, 16, 24
    x = np.random.default_rng(88).standard_normal((B, H, W)).astype(NP[dtype])
    blocks = x.reshape(B, H // 8, 8, W // 8, 8)
    ref = ref_nd(blocks, (2, 4), inverse, "ortho").reshape(B, H, W)
    # (the reference per block, the long way round, for the first and the last block)
    for b, i, j in ((0, 0, 0), (B - 1, H // 8 - 1, W // 8 - 1)):
        blk = x[b, 8 * i:8 * i + 8, 8 * j:8 * j + 8]
        assert np.abs(ref_nd(blk[None], (1, 2), inverse, "ortho")[0] - ref[b, 8 * i:8 * i + 8, 8 * j:8 * j + 8]).max() < 1e-12
    fn = mf.idctn if inverse else mf.dctn
    xd = torch.from_numpy(x).to(DEV)
    got = fn(xd.reshape(B, H // 8, 8, W // 8, 8), norm="ortho", dim=(2, 4)).reshape(B, H, W)
    err = _rel(got.cpu().numpy(), ref)
    assert err <= TOL[dtype], err


# ---- bin by bin --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("n", [16, 15])
def test_structured_input_bin_by_bin(n, dtype):
    """unit impulses in ONE real column and a different impulse in its pair partner, over the 8 columns of a (3, n, 8) tensor
    transformed along dim 1: a slip in the separating store (or the combining load of the inverse), or leakage between the two
    columns of a pair, would hide inside an L2 norm.  Every output element against the cosine formula, absolute tolerance
    TOL * sqrt(n) as test_gpu_dct.test_structured_input_bin_by_bin (inverse: scaled by 1 / 2n)."""
    tol = TOL[dtype]
    odd = 2 * (n // 6) + 1
    # (batch entry, row of the impulse, its column); the partner column of the pair gets -0.5 three rows further
    cases = ((0, 0, 2), (1, n - 1, 5), (2, odd, 0))
    x = np.zeros((3, n, 8), dtype=NP[dtype])
    want_f = np.zeros((3, n, 8))
    want_i = np.zeros((3, n, 8))
    k = np.arange(n)

    def fwd(j):
        return 2 * np.cos(np.pi * k * (2 * j + 1) / (2 * n))

    def inv(kk):
        return (np.ones(n) if kk == 0 else 2 * np.cos(np.pi * kk * (2 * k + 1) / (2 * n))) / (2 * n)

    for b, r, c in cases:
        partner, r2 = c ^ 1, (r + 3) % n
        x[b, r, c] = 1.0
        x[b, r2, partner] = -0.5
        want_f[b, :, c], want_f[b, :, partner] = fwd(r), -0.5 * fwd(r2)
        want_i[b, :, c], want_i[b, :, partner] = inv(r), -0.5 * inv(r2)
    got, plan = _run(x, dtype, inverse=False, axes=(1,))
    assert not np.isnan(got).any()
    assert plan.kernel_name(0).startswith(f"cols{n}_"), plan.kernel_name(0)
    d = np.abs(got - want_f)
    assert d.max() <= tol * np.sqrt(n), ("forward", np.unravel_index(d.argmax(), d.shape), d.max())
    back, _ = _run(x, dtype, inverse=True, axes=(1,))
    assert not np.isnan(back).any()
    d = np.abs(back - want_i)
    assert d.max() <= tol * np.sqrt(n) / (2 * n), ("inverse", np.unravel_index(d.argmax(), d.shape), d.max())


# ---- round trips -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(3, 30, 70), (2, 6, 15, 16)], ids=str)
def test_round_trips(shape, dtype, norm):
    tol = TOL[dtype]
    x = torch.randn(shape, dtype=dtype, device=DEV)
    X = mf.dctn(x, norm=norm)
    assert X.shape == x.shape and X.dtype == dtype
    xn, Xn = x.cpu().numpy(), X.cpu().numpy()
    assert _rel(mf.idctn(X, norm=norm).cpu().numpy(), xn) <= tol
    assert _rel(mf.dctn(mf.idctn(x, norm=norm), norm=norm).cpu().numpy(), xn) <= tol
    if norm == "ortho":  # Parseval
        b = shape[0]
        nx = np.linalg.norm(xn.astype(np.float64).reshape(b, -1), axis=1)
        nX = np.linalg.norm(Xn.astype(np.float64).reshape(b, -1), axis=1)
        assert (np.abs(nX - nx) <= tol * nx).all()


# ---- slabs -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["dctn", "idctn"])
@pytest.mark.parametrize("axes", [None, (1,)], ids=str)
def test_a_middle_slab_equals_the_same_rows_of_the_whole_batch(axes, inverse):
    x = np.random.default_rng(15).standard_normal((11, 15, 38)).astype(np.float32)
    whole, _ = _run(x, torch.float32, inverse=inverse, axes=axes)
    part, _ = _run(x, torch.float32, inverse=inverse, axes=axes, first=3, count=5)
    assert not np.isnan(whole).any()
    assert np.array_equal(part[3:8], whole[3:8])
    assert np.isnan(part[:3]).all() and np.isnan(part[8:]).all()


# ---- more than two rounds of the persistent grid ----------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["dct2", "dct3"])
def test_paired_columns_walk_three_rounds(inverse):
    """8-point columns over 83 pairs of columns (two tiles per batch entry, the second ragged), the batch sized from
    Plan.pass_geometry so that the persistent grid walks two full rounds and a partial one; the first, a middle and the last
    batch entries (tiles) against the reference, the whole output written and nothing behind it"""
    dtype, n, W = torch.float32, 8, 166

    def make(b):
        return mf.plan_fft(dtype, dtype, (b, n, W, 1), (b, n, W, 1), inverse=inverse, dctn=True, axes=(1,))

    probe = make(4)
    tile, threads, per4, G = probe.pass_geometry(0, FAR)
    per_entry = probe.pass_geometry(0, 4)[2] // 4
    assert per_entry >= 2 and (W // 2) % tile != 0, (tile, per_entry)
    B = -(-(2 * G + G // 2 + 3) // per_entry)
    while (B * per_entry) % G == 0 or (B * per_entry) % 8 == 0:
        B += 1
    plan = make(B)
    geo = plan.pass_geometry(0)
    text = f"{plan.kernel_name(0)}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} batch {B}"
    print(text)
    assert geo[:2] == (tile, threads) and geo[2] == B * per_entry, text
    assert geo[2] >= 2 * geo[3] + 1 and geo[2] % geo[3] != 0 and geo[2] % 8 != 0, text
    assert B * n * W * 4 <= (256 << 20), text
    x = torch.randn((B, n, W, 1), dtype=dtype, device=DEV)
    keep = x.clone()
    numel = B * n * W
    flat = torch.full((numel + 4096,), float("nan"), dtype=dtype, device=DEV)
    out = flat[:numel].view(B, n, W, 1)
    mf.fft(out, x, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "x was written"
    assert bool(torch.isnan(flat[numel:]).all()), "the guard behind the output was written"
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    idx = sorted({0, 1, B // 2 - 1, B // 2, B - 2, B - 1})
    it = torch.tensor(idx, device=DEV)
    got = out[it][..., 0].cpu().numpy()
    ref = ref_nd(x[it][..., 0].cpu().numpy(), (1,), inverse)
    err = _rel(got, ref)
    assert err <= TOL[dtype], (text, err)


# ---- alignment ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_base_pointer_aligned_to_one_element_only(dtype):
    """contiguous slices at a storage offset of 1 element on both sides: the paired-column tiles' two-real accesses are then
    aligned to one element only, the contract of include/mifft.h"""
    shape = (3, 15, 38)
    numel = int(np.prod(shape))
    big = torch.randn(1 + numel, dtype=dtype, device=DEV)
    x = big[1:].reshape(shape + (1,))
    assert x.is_contiguous() and x.data_ptr() % (2 * x.element_size()) != 0
    xn = x[..., 0].cpu().numpy()
    for inverse in (False, True):
        for axes in (None, (1,)):
            obig = torch.full((1 + numel + 64,), float("nan"), dtype=dtype, device=DEV)
            out = obig[1:1 + numel].reshape(shape + (1,))
            assert out.data_ptr() % (2 * out.element_size()) != 0
            plan = mf.plan_fft(dtype, dtype, x.shape, out.shape, inverse=inverse, dctn=True, axes=axes)
            mf.fft(out, x, plan=plan)
            torch.cuda.synchronize()
            assert torch.isnan(obig[:1]).all() and torch.isnan(obig[1 + numel:]).all()
            ref = ref_nd(xn, (1, 2) if axes is None else axes, inverse)
            assert _rel(out[..., 0].cpu().numpy(), ref) <= TOL[dtype], (inverse, axes)
    assert torch.equal(big[1:].reshape(shape), x[..., 0])


# ---- wrappers ----------------------------------------------------------------------------------------------------------------

def test_wrappers_shapes_dtypes_and_views():
    x = torch.randn(4, 6, 64, device=DEV)
    X = mf.dctn(x)
    assert X.shape == x.shape and X.dtype == torch.float32
    assert _rel(X.cpu().numpy(), ref_nd(x.cpu().numpy(), (1, 2))) <= REL_L2_TOL_F32
    Xd = mf.dctn(x, out_dtype=torch.float64, dim=(0, 2))  # dim 0 transformed: a batch of 1
    assert Xd.dtype == torch.float64
    assert _rel(Xd.cpu().numpy()[None], ref_nd(x.cpu().numpy(), (0, 2))[None]) <= REL_L2_TOL_F64
    y = mf.idctn(X, norm="ortho", out_dtype=torch.float64, dim=(-2, -1))
    assert y.dtype == torch.float64
    assert _rel(y.cpu().numpy(), ref_nd(X.cpu().numpy(), (1, 2), True, "ortho")) <= REL_L2_TOL_F64
    # size-1 dims do not count; an empty dim or one of size-1 dims only is a converted copy
    assert torch.equal(mf.dctn(x.unsqueeze(1)), X.unsqueeze(1))
    for dim in ((), (1,)):
        c = mf.dctn(x.unsqueeze(1), dim=dim, out_dtype=torch.float64)
        assert c.dtype == torch.float64 and torch.equal(c, x.unsqueeze(1).double())
    # a non-contiguous view gives what its contiguous copy gives
    base = torch.randn(6, 5, 30, 16, device=DEV)
    view = base.transpose(0, 1)[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(mf.dctn(view), mf.dctn(view.contiguous()))
    assert torch.equal(mf.idctn(view, norm="ortho", dim=(2,)), mf.idctn(view.contiguous(), norm="ortho", dim=(2,)))
    # dct / idct keep their refusal of a dim that is not the innermost
    with pytest.raises(mf.MifftError) as e:
        mf.dct(x, dim=1)
    assert e.value.status == -15
    # layouts the library refuses, with its reason
    with pytest.raises(mf.MifftError) as e:
        mf.dctn(torch.randn(3, 8, 7, device=DEV), dim=(1,))  # an odd stride
    assert e.value.status == -15 and "odd stride" in str(e.value)
    with pytest.raises(mf.MifftError) as e:
        mf.dctn(torch.randn(3, 8, 2, device=DEV), dim=(1,))  # a single pair of columns
    assert e.value.status == -15 and "stride of 2" in str(e.value)


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.float16], ids=str)
def test_narrow_input_types(in_dtype):
    """a narrow input goes to the plan when the last dim is transformed (the row pass widens it) and is widened first otherwise"""
    shape = (3, 16, 64)
    rng = np.random.default_rng(7)
    if in_dtype == torch.uint8:
        xt = torch.from_numpy(rng.integers(0, 256, size=shape).astype(np.uint8))
    else:
        xt = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(in_dtype)
    wide = xt.to(torch.float64).numpy()
    got, plan = _run(xt.float().numpy(), torch.float32, inverse=False, in_dtype=in_dtype)
    assert plan.in_dtype == in_dtype
    assert _rel(got, ref_nd(wide, (1, 2))) <= REL_L2_TOL_F32
    y = mf.dctn(xt.to(DEV))
    assert y.dtype == torch.float64 and _rel(y.cpu().numpy(), ref_nd(wide, (1, 2))) <= REL_L2_TOL_F64
    y = mf.dctn(xt.to(DEV), dim=(1,), out_dtype=torch.float32)  # the column pass first: widened by the wrapper
    assert y.dtype == torch.float32 and _rel(y.cpu().numpy(), ref_nd(wide, (1,))) <= REL_L2_TOL_F32
    with pytest.raises(mf.MifftError) as e:  # ... which a plan refuses
        mf.plan_fft(in_dtype, torch.float32, shape + (1,), shape + (1,), dctn=True, axes=(1,))
    assert e.value.status == -15 and "in_dtype" in str(e.value)


# ---- introspection -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_introspection(dtype):
    esz = 4 if dtype == torch.float32 else 8
    f64 = "f64_" if dtype == torch.float64 else ""
    shape = (5, 30, 64, 1)
    for inverse, tag in ((False, "dct2"), (True, "dct3")):
        plan = mf.plan_fft(dtype, dtype, shape, shape, inverse=inverse, dctn=True)
        assert plan.num_launches == 2 and plan.scratch_bytes == 0
        assert plan.in_bytes == plan.out_bytes == 5 * 30 * 64 * esz
        rows, cols = plan.kernel_name(1), plan.kernel_name(0)
        assert rows.startswith(f"rows64_{f64}{tag}_"), rows
        assert cols.startswith(f"cols30_{f64}{tag}_") and cols.endswith("_jit"), cols
        assert int(np.prod(plan.stages(1))) == 32, plan.stages(1)  # the packed n / 2-point transform of the rows
        assert int(np.prod(plan.stages(0))) == 30, plan.stages(0)
        tile, threads, n_tiles, grid = plan.pass_geometry(0)
        assert n_tiles == 5 * -(-32 // tile) and 1 <= grid <= n_tiles and threads % 64 == 0
        assert plan.pass_geometry(1)[2] >= 1
        # a kept dim between: no stages, no kernel, no pass
        kshape = (5, 8, 6, 8, 1)
        kplan = mf.plan_fft(dtype, dtype, kshape, kshape, inverse=inverse, dctn=True, axes=(1, 3), norm="ortho")
        assert kplan.num_launches == 2 and kplan.scratch_bytes == 0
        assert kplan.stages(1) == [] and kplan.kernel_name(1) == "none"
        assert kplan.kernel_name(0).startswith(f"cols8_{f64}{tag}_") and kplan.kernel_name(2).startswith(f"rows8_{f64}{tag}_")
        assert kplan.in_bytes == kplan.out_bytes == 5 * 8 * 6 * 8 * esz


# ---- MIFFT_JIT=0 -------------------------------------------------------------------------------------------------------------

def test_without_runtime_specialisation_a_column_pass_is_refused():
    """MIFFT_JIT=0 (a fresh process, with its own time limit): a 2-D plan is refused with the reason -- its column tiles are
    compiled at run time only -- while mf.dct of 1024 points still plans"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "import hackathon_fft_amd as mf\n"
            "try:\n"
            "    mf.dctn(torch.zeros(2, 64, 1024, device='cuda:0'))\n"
            "    print('planned')\n"
            "except mf.MifftError as e:\n"
            "    print('refused', e.status, 'MIFFT_JIT=0' in str(e))\n"
            "y = mf.dct(torch.ones(2, 1024, device='cuda:0'))\n"
            "torch.cuda.synchronize()\n"
            "print('dct', tuple(y.shape), float(y[0, 0]))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIFFT_JIT="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines == ["refused -15 True", "dct (2, 1024) 2048.0"], r.stdout
