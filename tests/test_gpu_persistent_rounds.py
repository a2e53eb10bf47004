"""The packed-row (TileCfg::R2C / C2R), DCT (TileCfg::DCT) and interleaved (TileCfg::ILV) tile kernels beyond one tile per
workgroup: every case is sized from Plan.pass_geometry so that the persistent grid walks two full rounds plus a partial one with
a ragged last tile, and EVERY output row is compared with an fp64 numpy reference.  Also the two size-dependent twins that no
other test executes: the DCT-II rows with non-temporal loads (`_ntl`) and the interleaved tile's `_nt` twin.

The GPU tests carry the gpu mark one by one (not a module-wide pytestmark): the pin of the DCT reference used here to the one
of test_gpu_dct.py is host-only and runs without a device."""
import ctypes

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_gpu_dct import _ortho_scale, ref_dct, ref_idct

gpu = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: REL_L2_TOL_F32, torch.float64: REL_L2_TOL_F64}
# two kernels with the same arithmetic (conftest.check_hermitian_plan's figures)
TWIN_TOL = {torch.float32: 2e-6, torch.float64: 1e-12}
NP = {torch.float32: np.float32, torch.float64: np.float64}
CNP = {torch.float32: np.complex64, torch.float64: np.complex128}
DT = {"f32": torch.float32, "f64": torch.float64}
GUARD = 4096           # NaN elements behind every output
MAX_BYTES = 512 << 20  # per tensor
FAR = 1 << 40          # a count at which no grid is clamped by the tile count
CHUNK = 2048           # rows per call of the CPU reference


# ---- references ------------------------------------------------------------------------------------------------------------

def ref2_dct(x, norm=None):
    """scipy.fft.dct(x, 2, norm) of the rows of x in fp64 by the 2n-point even extension:
    X[k] = Re(exp(-i pi k / 2n) rfft([x, x[::-1]])[k]) (a quarter of the points of test_gpu_dct.ref_dct)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    Y = np.fft.rfft(np.concatenate([x, x[..., ::-1]], axis=-1), axis=-1)[..., :n]
    X = (np.exp(-1j * np.pi * np.arange(n) / (2 * n)) * Y).real
    return X * _ortho_scale(n) if norm == "ortho" else X


def ref2_idct(X, norm=None):
    """scipy.fft.idct(X, 2, norm) in fp64: irfft of exp(i pi k / 2n) X[k] with a zero bin at n, first n samples"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[-1]
    if norm == "ortho":
        X = X / _ortho_scale(n)
    Z = np.zeros(X.shape[:-1] + (n + 1,), dtype=np.complex128)
    Z[..., :n] = np.exp(1j * np.pi * np.arange(n) / (2 * n)) * X
    return np.fft.irfft(Z, n=2 * n, axis=-1)[..., :n]


def test_the_2n_point_dct_reference_equals_the_4n_point_one():
    """host only: the quicker route used in this file against ref_dct / ref_idct of test_gpu_dct.py, to 1e-14 of the largest
    value"""
    rng = np.random.default_rng(5)
    for n in (8, 30, 1024):
        x = rng.standard_normal((6, n))
        for norm in (None, "ortho"):
            a, b = ref2_dct(x, norm), ref_dct(x, norm)
            assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max(), (n, norm)
            a, b = ref2_idct(x, norm), ref_idct(x, norm)
            assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max(), (n, norm)


def test_pass_geometry_refuses_a_null_plan_or_buffer():
    """host only: the query's argument checks need no device"""
    L = _lib.lib()
    g = (ctypes.c_int64 * 4)()
    assert L.mifft_plan_pass_geometry(None, 0, 1, g) == -12
    assert L.mifft_last_error()


def _as_rows(a):
    """(b, ..) real or complex -> (b, m) float64, complex numbers as interleaved pairs"""
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        a = a.astype(np.complex128).view(np.float64)
    return a.astype(np.float64, copy=False).reshape(a.shape[0], -1)


def _cplx(a):
    """interleaved (.., 2) -> complex128"""
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


# ---- sizing ----------------------------------------------------------------------------------------------------------------

def _geo_text(name, geo, rows):
    return f"{name}: tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]} rows {rows}"


def _rounds_ok(geo, rows, unit=1):
    """the sizing rule on a geometry: two full rounds and a partial one, no whole number of rounds or of XCD chunks, a ragged
    last tile (rows None: a pass whose tiles are not runs of rows).  unit: the transforms that come and go together -- 1 row,
    or the I transforms of an interleaved block, whose tiles are whole blocks: a tile of ONE unit cannot be ragged."""
    tile, _, n_tiles, grid = geo
    return (n_tiles >= 2 * grid + 1 and n_tiles % grid != 0 and n_tiles % 8 != 0 and
            (rows is None or tile <= unit or rows % tile != 0))


def _size_rows(probe, per_entry=1):
    """batch entries (of per_entry transforms each) for the single pass of `probe`, and the probe's (tile, threads)"""
    tile, threads, _, G = probe.pass_geometry(0, FAR)
    n_tiles = 2 * G + G // 2 + 3
    while n_tiles % 8 == 0 or n_tiles % G == 0:
        n_tiles += 1
    rows = (n_tiles - 1) * tile + max(1, tile // 3)
    B = -(-rows // per_entry)
    for _ in range(4096):  # (per_entry > 1: the smallest batch from there that keeps the rule)
        if _rounds_ok((tile, threads, -(-B * per_entry // tile), G), B * per_entry, per_entry):
            break
        B += 1
    return B, (tile, threads)


def _assert_rounds(plan, dim, probe_tt, rows, what, unit=1):
    geo = plan.pass_geometry(dim)
    text = _geo_text(what + " " + plan.kernel_name(dim), geo, rows)
    tile, threads, n_tiles, grid = geo
    assert n_tiles >= 2 * grid + 1, text
    assert n_tiles % grid != 0, text
    assert n_tiles % 8 != 0, text
    if rows is not None and tile > unit:
        assert rows % tile != 0, text
    assert (tile, threads) == tuple(probe_tt), (text, probe_tt)
    return geo


# ---- running ---------------------------------------------------------------------------------------------------------------

def _exec_guarded(plan, x, first=None, count=None):
    """exec into a NaN-prefilled output with GUARD more NaN elements behind it, which must stay NaN"""
    numel = int(np.prod(plan.out_shape))
    assert numel * x.element_size() <= MAX_BYTES and x.numel() * x.element_size() <= MAX_BYTES, (plan.in_shape, plan.out_shape)
    flat = torch.full((numel + GUARD,), float("nan"), dtype=plan.out_dtype, device=DEV)
    out = flat[:numel].view(plan.out_shape)
    if first is None:
        mf.fft(out, x, plan=plan)
    else:
        mf.fft(out, x, plan=plan, first=first, count=count)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[numel:]).all()), "the guard behind the output was written"
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check_rounds(what, plan, geos, x_np, ref_rows, to_rows, per_entry=1):
    """whole exec + every row against the reference + the slab contract in the last round.  geos: {dim: geometry} of the
    passes that answered (already asserted); the FIRST one names the tile / round of a failing row.  ref_rows(x chunk) and
    to_rows(output chunk) give (transforms of the chunk, m) float64."""
    dtype = plan.out_dtype
    B = plan.out_shape[0]
    rows = B * per_entry
    dim0 = next(iter(geos))
    tile, threads, n_tiles, grid = geos[dim0]
    x = torch.from_numpy(x_np).to(DEV)
    keep = x.clone()
    out = _exec_guarded(plan, x)
    assert torch.equal(_bits(x), _bits(keep)), "x was written"
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    got = out.cpu().numpy()
    worst, worst_row = 0.0, 0
    step = max(1, CHUNK // per_entry)
    for lo in range(0, B, step):
        g = to_rows(got[lo:lo + step])
        r = ref_rows(x_np[lo:lo + step])
        assert g.shape == r.shape, (g.shape, r.shape)
        e = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
        k = int(e.argmax())
        if e[k] > worst:
            worst, worst_row = float(e[k]), lo * per_entry + k
    for d, geo in geos.items():
        print(_geo_text(f"{what} dim {d} {plan.kernel_name(d)}", geo, rows), f"worst rel-L2 {worst:.3e}")
    assert worst <= TOL[dtype], (what, f"row {worst_row} tile {worst_row // tile} round {worst_row // tile // grid}", worst)
    # a slab that starts inside a tile of the last round and crosses a tile boundary: bit for bit the same rows, nothing else
    if tile > 1:
        r0, rc = rows - tile - tile // 2 - 1, tile + 1
    else:
        r0, rc = rows - 4, 3
    first = r0 // per_entry
    count = min(B - first, -(-(r0 + rc) // per_entry) - first)
    assert first > 0 and count > 0 and first + count <= B
    part = _exec_guarded(plan, x, first=first, count=count)
    assert torch.equal(_bits(part[first:first + count]), _bits(out[first:first + count])), (what, "slab differs", first, count)
    assert bool(torch.isnan(part[:first]).all()) and bool(torch.isnan(part[first + count:]).all()), (what, "slab wrote outside")
    assert torch.equal(_bits(x), _bits(keep)), "x was written"


def _rng_real(seed, shape, dtype):
    return np.random.default_rng(seed).standard_normal(shape).astype(NP[dtype])


LENGTHS = {"f32": [8, 30, 480, 1024, 16384], "f64": [8, 30, 480, 1024, 8192]}
ROW_CASES = [(n, t) for t in ("f32", "f64") for n in LENGTHS[t]]


# ---- packed real rows --------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("inverse", [False, True], ids=["r2c", "c2r"])
@pytest.mark.parametrize("n,t", ROW_CASES, ids=lambda v: str(v))
def test_packed_rows_walk_three_rounds(n, t, inverse):
    dtype = DT[t]
    h = n // 2 + 1

    def shapes(b):
        real, half = (b, n, 1), (b, h, 2)
        return (half, real) if inverse else (real, half)

    def make(b):
        return mf.plan_fft(dtype, dtype, *shapes(b), inverse=inverse, half_spectrum=True)

    B, probe_tt = _size_rows(make(4))
    plan = make(B)
    assert ("_c2r_" if inverse else "_r2c_") in plan.kernel_name(0), plan.kernel_name(0)
    geo = _assert_rounds(plan, 0, probe_tt, B, f"packed {n} {t}")
    x = _rng_real(n * 4 + inverse, shapes(B)[0], dtype)
    if inverse:  # arbitrary complex bins: the imaginary parts of bins 0 and n / 2 are nonzero and must be ignored
        ref = lambda c: _as_rows(np.fft.irfft(_cplx(c), n=n, axis=-1))
    else:
        ref = lambda c: _as_rows(np.fft.rfft(c[..., 0].astype(np.float64), axis=-1))
    _check_rounds(f"packed {n} {t} inverse={inverse}", plan, {0: geo}, x, ref, _as_rows)


# ---- DCT rows ----------------------------------------------------------------------------------------------------------------

DCT_CASES = [(n, t, None) for n, t in ROW_CASES] + [(1024, "f32", "ortho")]


@gpu
@pytest.mark.parametrize("inverse", [False, True], ids=["dct2", "dct3"])
@pytest.mark.parametrize("n,t,norm", DCT_CASES, ids=lambda v: str(v))
def test_dct_rows_walk_three_rounds(n, t, norm, inverse):
    dtype = DT[t]

    def make(b):
        return mf.plan_fft(dtype, dtype, (b, n, 1), (b, n, 1), inverse=inverse, dct=True, norm=norm)

    B, probe_tt = _size_rows(make(4))
    plan = make(B)
    assert ("_dct3_" if inverse else "_dct2_") in plan.kernel_name(0), plan.kernel_name(0)
    geo = _assert_rounds(plan, 0, probe_tt, B, f"dct {n} {t}")
    x = _rng_real(n * 4 + 2 + inverse, (B, n, 1), dtype)
    fn = ref2_idct if inverse else ref2_dct
    _check_rounds(f"dct {n} {t} norm={norm} inverse={inverse}", plan, {0: geo}, x, lambda c: fn(c[..., 0], norm), _as_rows)


# ---- interleaved block tile --------------------------------------------------------------------------------------------------

ILV_CASES = [(N, I, t) for t in ("f32", "f64") for N, I in ((93, 2), (128, 3), (480, 4), (1024, 2))] + \
            [(128, 15, "f32"), (128, 7, "f64")]


def _ilv_rows(o):
    """(b, N, I, 2) -> one row per transform, (b * I, 2 N)"""
    return _as_rows(np.ascontiguousarray(o.transpose(0, 2, 1, 3)).reshape(o.shape[0] * o.shape[2], -1))


@gpu
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("N,I,t", ILV_CASES, ids=lambda v: str(v))
def test_interleaved_tile_walks_three_rounds(N, I, t, inverse):
    dtype = DT[t]

    def make(b):
        return mf.plan_fft(dtype, dtype, (b, N, I, 2), (b, N, I, 2), inverse=inverse, axes=(1,))

    B, probe_tt = _size_rows(make(4), per_entry=I)
    plan = make(B)
    assert plan.kernel_name(0).startswith(f"ilv{N}x{I}_"), plan.kernel_name(0)
    geo = _assert_rounds(plan, 0, probe_tt, B * I, f"ilv {N}x{I} {t}", unit=I)
    x = _rng_real(N * 16 + I * 2 + inverse, (B, N, I, 2), dtype)
    f = np.fft.ifft if inverse else np.fft.fft

    def ref(c):
        y = f(_cplx(c), axis=1)  # (b, N, I)
        return _as_rows(np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(y.shape[0] * I, N))

    _check_rounds(f"ilv {N}x{I} {t} inverse={inverse}", plan, {0: geo}, x, ref, _ilv_rows, per_entry=I)


# ---- N-D half spectrum -------------------------------------------------------------------------------------------------------

def _answering(plan, count=None):
    geos = {}
    for d in range(plan.ndim):
        try:
            geos[d] = plan.pass_geometry(d, count)
        except mf.MifftError as e:
            assert e.status == -15, e
    return geos


@gpu
@pytest.mark.parametrize("dims,inverse", [((48, 40), False), ((48, 40), True), ((16, 24, 32), True)], ids=lambda v: str(v))
def test_nd_half_spectrum_walks_three_rounds(dims, inverse):
    dtype = torch.float32
    n, nd = dims[-1], len(dims)
    lead = int(np.prod(dims[:-1]))  # rows of the last dimension per batch entry

    def shapes(b):
        real, half = (b,) + dims + (1,), (b,) + dims[:-1] + (n // 2 + 1, 2)
        return (half, real) if inverse else (real, half)

    def make(b):
        return mf.plan_fft(dtype, dtype, *shapes(b), inverse=inverse, half_spectrum=True)

    def rows_of(d, b, tile):  # only the packed rows of the last dimension are tiles of whole rows, and only when a batch
        return b * lead if d == nd - 1 and lead % tile != 0 else None  # entry is no whole number of tiles can one be ragged

    probe = make(4)
    far = _answering(probe, FAR)
    assert nd - 1 in far, ("the packed rows do not answer", far)
    dmax = max(far, key=lambda d: far[d][3])  # size by the pass with the largest grid ...
    G = far[dmax][3]
    per_entry_tiles = probe.pass_geometry(dmax, 1024)[2] / 1024.0
    B = max(5, int((2 * G + G // 2 + 3) / per_entry_tiles))
    for _ in range(4096):  # ... then the smallest batch from there at which EVERY answering pass keeps the rule
        if all(_rounds_ok(g, rows_of(d, B, g[0])) for d, g in _answering(probe, B).items()):
            break
        B += 1
    plan = make(B)
    geos = {}
    for d in sorted(far, key=lambda d: d != nd - 1):  # (the packed rows first: they name a failing row's tile)
        geos[d] = _assert_rounds(plan, d, far[d][:2], rows_of(d, B, far[d][0]), f"nd {dims} dim {d}")
    x = _rng_real(sum(dims) + inverse, shapes(B)[0], dtype)
    axes = tuple(range(1, nd + 1))
    if inverse:
        ref = lambda c: _as_rows(np.fft.irfftn(_cplx(c), s=dims, axes=axes))
    else:
        ref = lambda c: _as_rows(np.fft.rfftn(c[..., 0].astype(np.float64), axes=axes))
    _check_rounds(f"nd {dims} inverse={inverse}", plan, geos, x, ref, _as_rows)


# ---- streaming twins ---------------------------------------------------------------------------------------------------------

TWIN_BYTES = 0.70e9   # in + out of the plan that must take the twin (the threshold is 0.60e9)
PLAIN_BYTES = 0.27e9  # ... and of the slab plan that must not (below 0.3e9)


def _sample(B, tile, n_tiles, per_entry, n=256):
    """n batch entries: those of the first tile, those of the last (ragged) tile and an even stride between them"""
    head = np.arange(min(B, -(-tile // per_entry)))
    tail = np.arange((n_tiles - 1) * tile // per_entry, B)
    mid = np.linspace(len(head), tail[0], max(2, n - len(head) - len(tail)), endpoint=False).astype(np.int64)
    return np.unique(np.concatenate([head, mid, tail]))


def _check_twin(what, make, entry_bytes, per_entry, is_twin, ref_rows, to_rows, dtype):
    """make(b) -> plan of b batch entries of entry_bytes (in + out).  The twin's whole output against the plain kernel's (a
    sub-threshold plan looped over slabs of the same input), row by row on the device in fp64; 256 entries against numpy."""
    B = int(TWIN_BYTES / entry_bytes) // 64 * 64 + 64 + 5  # (ragged for every tile that divides 64)
    slab = int(PLAIN_BYTES / entry_bytes)
    twin, plain = make(B), make(slab)
    assert is_twin(twin.kernel_name(0)), twin.kernel_name(0)
    assert not is_twin(plain.kernel_name(0)), plain.kernel_name(0)
    geo = twin.pass_geometry(0)
    tile, _, n_tiles, grid = geo
    assert n_tiles >= 2 * grid + 1 and (tile == 1 or (B * per_entry) % tile != 0), _geo_text(what, geo, B * per_entry)
    x = torch.randn(twin.in_shape, dtype=twin.in_dtype, device=DEV)
    keep = x.clone()
    out = _exec_guarded(twin, x)
    assert torch.equal(_bits(x), _bits(keep)), "x was written"
    del keep
    assert not bool(torch.isnan(out).any())
    numel = int(np.prod(twin.out_shape))
    flat = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device=DEV)
    base = flat[:numel].view(twin.out_shape)
    for s in range(0, B, slab):
        s = min(s, B - slab)  # (the last slab overlaps its predecessor: slabs are bit-identical wherever they start)
        mf.fft(base[s:s + slab], x[s:s + slab], plan=plain)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[numel:]).all()) and not bool(torch.isnan(base).any())
    worst = 0.0
    for lo in range(0, B, 8192):
        a, b = to_rows(out[lo:lo + 8192].double()), to_rows(base[lo:lo + 8192].double())
        e = (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)
        worst = max(worst, float(e.max()))
    same = torch.equal(_bits(out), _bits(base))
    idx = _sample(B, tile, n_tiles, per_entry)
    it = torch.from_numpy(idx).to(DEV)
    g = to_rows(out[it].double()).cpu().numpy()
    r = ref_rows(x[it].cpu().numpy())
    err = float((np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)).max())
    print(_geo_text(f"{what} {twin.kernel_name(0)} (plain: {plain.kernel_name(0)}, {slab} entries)", geo, B * per_entry),
          f"twin vs plain worst rel-L2 {worst:.3e} bit-identical {same}; {len(idx)} entries vs numpy {err:.3e}")
    assert worst <= TWIN_TOL[dtype], (what, worst)
    assert err <= TOL[dtype], (what, err)


@gpu
@pytest.mark.parametrize("n,t,suffix", [(1024, "f32", "_ntl"), (1024, "f64", "_ntl"), (480, "f32", "_ntl_jit")], ids=str)
def test_dct2_streaming_twin_equals_the_plain_kernel(n, t, suffix):
    dtype = DT[t]
    esz = 4 if t == "f32" else 8
    make = lambda b: mf.plan_fft(dtype, dtype, (b, n, 1), (b, n, 1), dct=True)
    flat = lambda o: o.reshape(o.shape[0], -1)
    _check_twin(f"dct2 {n} {t}", make, 2 * n * esz, 1, lambda name: name.endswith(suffix),
                lambda c: ref2_dct(c[..., 0]), flat, dtype)


@gpu
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_interleaved_streaming_twin_equals_the_plain_kernel(inverse):
    N, I, dtype = 1024, 2, torch.float32
    make = lambda b: mf.plan_fft(dtype, dtype, (b, N, I, 2), (b, N, I, 2), inverse=inverse, axes=(1,))
    f = np.fft.ifft if inverse else np.fft.fft

    def ref(c):
        y = f(_cplx(c), axis=1)
        return _as_rows(np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(y.shape[0] * I, N))

    def rows(o):  # (b, N, I, 2) on the device -> (b * I, 2 N)
        return o.permute(0, 2, 1, 3).reshape(o.shape[0] * I, -1)

    def is_twin(name):
        assert name.startswith(f"ilv{N}x{I}_"), name
        return "_nt" in name

    _check_twin(f"ilv {N}x{I} inverse={inverse}", make, 2 * N * I * 8, I, is_twin, ref, rows, dtype)
