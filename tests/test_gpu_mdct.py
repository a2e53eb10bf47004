"""The fused MDCT on the MI355X (MIFFT_MDCT_TAG): the TileCfg::MDCT kernel against the direct definition over zero-padded
frames in fp64 (test_mdct_host.ref_mdct), and imdct -- a composition of one DCT-IV launch and torch -- against the signal."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_dct4_host import ref_dct4
from test_mdct_host import ref_mdct

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
NP = {torch.float32: np.float32, torch.float64: np.float64}
NORMS = [None, "ortho"]
GUARD = 4096  # NaN elements behind every output
FAR = 1 << 20


def _rel(got, ref):
    """max over the rows -- here: the frames -- of ||got - ref|| / ||ref||"""
    g = np.asarray(got, dtype=np.float64).reshape(-1, got.shape[-1])
    r = np.asarray(ref, dtype=np.float64).reshape(-1, ref.shape[-1])
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())


def _fold(frames, n):
    """the 2n windowed samples of every frame folded to the n values whose DCT-IV is twice the MDCT"""
    ia, sa, ib, sb = (t.numpy() for t in mf.api._mdct_fold_tables(n))
    return sa * frames[..., ia] + sb * frames[..., ib]


def _frames(x, n, w):
    """the zero-padded, windowed frames of x (B, T): (B, F, 2n) in fp64"""
    x = np.asarray(x, dtype=np.float64)
    B, T = x.shape
    F = mf.mdct_frames(T, n)
    xp = np.zeros((B, (F + 1) * n))
    xp[:, n:n + T] = x
    return np.stack([xp[:, f * n:f * n + 2 * n] for f in range(F)], axis=1) * np.asarray(w, dtype=np.float64)


def _ref(x, n, w, norm):
    """the definition (the cosine matrix) up to 1080 coefficients; beyond, the fold and the DCT-IV reference, which
    test_mdct_host.py checks against the definition"""
    if n <= 1080:
        return ref_mdct(x, n, w, norm)
    X = ref_dct4(_fold(_frames(x, n, w), n)) / 2
    return X * np.sqrt(2.0 / n) if norm == "ortho" else X


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_guarded(plan, x, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN; x must not change.
    Returns the output (B, F, n) as float64 on the host."""
    numel = int(np.prod(plan.out_shape))
    flat = torch.full((numel + GUARD,), float("nan"), dtype=plan.out_dtype, device=DEV)
    out = flat[:numel].view(plan.out_shape)
    before = x.clone()
    if first is None:
        mf.fft(out, x, plan=plan)
    else:
        mf.fft(out, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert torch.isnan(flat[numel:]).all(), "the guard region behind the output was written"
    assert torch.equal(_bits(x), _bits(before)), "x was written"
    return out.cpu().numpy()[..., 0].astype(np.float64)


def _window(kind, n, seed):
    if kind == "sine":
        return None
    return np.random.default_rng(seed).uniform(0.25, 1.0, 2 * n) * np.random.default_rng(seed + 1).choice([-1.0, 1.0], 2 * n)


# (batch, T, n), fp64 too?
SHAPES = [((3, 100, 8), True),
          ((5, 1000, 16), True),
          ((4, 333, 30), True),      # odd h: the middle pairs straddle a quarter boundary
          ((3, 4096, 256), True),    # n divides T
          ((2, 5000, 1024), True),
          ((7, 5, 8), True),         # T < n: F = 2 and both frames reach past both ends
          ((2, 40000, 8192), False)]
CASES = [(s, torch.float32) for s, _ in SHAPES] + [(s, torch.float64) for s, f64 in SHAPES if f64]


@pytest.mark.parametrize("window", ["sine", "random"])
@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v))
def test_matches_the_definition(shape, dtype, norm, window):
    B, T, n = shape
    rng = np.random.default_rng(B + T + n)
    xh = rng.standard_normal((B, T)).astype(NP[dtype])
    w = _window(window, n, n)
    plan = mf.plan_mdct(dtype, B, T, n, window=w, norm=norm)
    F = mf.mdct_frames(T, n)
    assert plan.in_shape == (B, T, 1) and plan.out_shape == (B, F, n, 1)
    name = plan.kernel_name(1)
    assert "_dct4_" in name and name.endswith("_mdct_jit") and name.startswith(f"rows{n}_"), name
    assert plan.kernel_name(0) == "none" and plan.stages(0) == [] and int(np.prod(plan.stages(1))) == n // 2
    assert plan.num_launches == 1 and plan.scratch_bytes == 0
    es = 4 if dtype == torch.float32 else 8
    assert plan.in_bytes == B * T * es and plan.out_bytes == B * F * n * es
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    assert not np.isnan(got).any()
    err = _rel(got, _ref(xh, n, mf.mdct_window(n).numpy() if w is None else w, norm))
    print(f"mdct {shape} {dtype} norm={norm} window={window}: frame rel L2 {err:.3e} {name} geometry={plan.pass_geometry(1)}")
    assert err <= TOL[dtype], (shape, err, name)
    plan.close()


@pytest.mark.parametrize("n,T", [(16, 100), (30, 333)])
def test_a_slab_exec_touches_its_own_entries_only(n, T):
    """first = 2, count = 2 of a batch of 5: the other entries are NaN in x and stay NaN in out, nothing behind out is written,
    and the slab's frames are bit-identical to the same frames of the whole batch"""
    B = 5
    xh = np.random.default_rng(10).standard_normal((B, T)).astype(np.float32)
    ref = ref_mdct(xh, n)
    plan = mf.plan_mdct(torch.float32, B, T, n)
    whole = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    xh[[0, 1, 4]] = np.nan
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1), first=2, count=2)
    assert np.isnan(got[[0, 1, 4]]).all()
    assert not np.isnan(got[2:4]).any()
    assert np.array_equal(got[2:4], whole[2:4])
    assert _rel(got[2:4], ref[2:4]) <= REL_L2_TOL_F32
    # the same entries through a plan of their own batch: a frame's result does not depend on batch or grid
    small = mf.plan_mdct(torch.float32, 2, T, n)
    alone = _exec_guarded(small, torch.from_numpy(np.ascontiguousarray(xh[2:4])).to(DEV).reshape(2, T, 1))
    assert np.array_equal(alone, whole[2:4])
    plan.close()
    small.close()


def test_persistent_rounds_and_tiles_that_straddle_entries():
    """n = 256, T = 1000 (F = 5, no multiple of the tile), sized from pass_geometry(1) so that every workgroup walks more than
    one tile, the last tile is ragged and tiles straddle entry boundaries; every frame is compared"""
    n, T = 256, 1000
    F = mf.mdct_frames(T, n)
    assert F == 5
    probe = mf.plan_mdct(torch.float32, 1, T, n)
    tile, threads, _, G = probe.pass_geometry(1, FAR)
    probe.close()
    assert tile > 1 and tile % F != 0, (tile, F)

    def ok(B):
        rows = B * F
        n_tiles = -(-rows // tile)
        return n_tiles >= 2 * G + 1 and n_tiles % G != 0 and rows % tile != 0

    B = -(-((2 * G + G // 2 + 3) * tile) // F)
    while not ok(B):
        B += 1
    plan = mf.plan_mdct(torch.float32, B, T, n)
    geo = plan.pass_geometry(1)
    text = f"{plan.kernel_name(1)}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {B * F}"
    print(text)
    assert (geo[0], geo[1]) == (tile, threads) and geo[2] == -(-B * F // tile) and geo[3] == G, text
    xh = np.random.default_rng(9).standard_normal((B, T)).astype(np.float32)
    got = _exec_guarded(plan, torch.from_numpy(xh).to(DEV).reshape(B, T, 1))
    assert not np.isnan(got).any()
    err = 0.0
    for b0 in range(0, B, 1024):  # (the reference in chunks)
        err = max(err, _rel(got[b0:b0 + 1024], ref_mdct(xh[b0:b0 + 1024], n)))
    print(f"mdct persistent rounds B={B}: frame rel L2 {err:.3e}")
    assert err <= REL_L2_TOL_F32
    plan.close()


@pytest.mark.parametrize("norm", NORMS, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape,n", [((3, 1024), 64), ((2, 3, 1000), 64), ((700,), 30)], ids=str)
def test_imdct_of_mdct_reproduces_the_signal(shape, n, dtype, norm):
    """the sine window on both sides (TDAC), T a multiple of n and not"""
    x = torch.randn(shape, dtype=dtype, device=DEV)
    X = mf.mdct(x, n, norm=norm)
    T = shape[-1]
    F = mf.mdct_frames(T, n)
    assert X.shape == shape[:-1] + (F, n) and X.dtype == dtype and X.is_contiguous()
    y = mf.imdct(X, norm=norm, length=T)
    assert y.shape == x.shape and y.dtype == dtype
    xn = x.cpu().numpy().reshape(-1, T)
    assert _rel(y.cpu().numpy().reshape(-1, T), xn) <= TOL[dtype]
    full = mf.imdct(X, norm=norm)  # length defaults to (F - 1) n: the signal, then the zeros the last frames saw
    L = (F - 1) * n
    assert full.shape[-1] == L
    padded = np.zeros((xn.shape[0], L))
    padded[:, :T] = xn
    assert _rel(full.cpu().numpy().reshape(-1, L), padded) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [30, 256])
def test_equals_the_dct4_of_frames_folded_on_the_host(n, dtype):
    B, T = 3, 7 * n + 11
    xh = np.random.default_rng(n).standard_normal((B, T)).astype(NP[dtype])
    w = _window("random", n, 3)
    got = mf.mdct(torch.from_numpy(xh).to(DEV), n, window=w).cpu().numpy()
    u = _fold(_frames(xh, n, w), n)
    twin = mf.dct(torch.from_numpy(u.astype(NP[dtype])).to(DEV), type=4).cpu().numpy() / 2
    # u is rounded once more on the twin's side: two roundings of the plan's float type on top of the transform's own error
    eps = float(np.finfo(NP[dtype]).eps)
    assert _rel(got, twin) <= TOL[dtype] + 2 * eps
    assert _rel(got, ref_mdct(xh, n, w)) <= TOL[dtype]


def test_a_window_changed_in_place_never_meets_a_stale_plan():
    n = 16
    x = torch.randn(2, 200, device=DEV)
    w = mf.mdct_window(n).clone()
    a = mf.mdct(x, n, window=w)
    w.mul_(2.0)
    b = mf.mdct(x, n, window=w)
    assert _rel(b.cpu().numpy(), 2 * a.cpu().numpy().astype(np.float64)) <= REL_L2_TOL_F32
    assert torch.equal(mf.mdct(x, n), mf.mdct(x, n, window=mf.mdct_window(n)))
