"""One column length per configuration CLASS of the column tiles, through the paired-column DCT / DST kernels and the plain
complex column pass of a kept-dim plan.

choose_config(n, cols=true, ..) (csrc/kernels_jit.cpp) derives from the column length, the float type and the stride the radix
list (one to four passes, a three-pass re-choice for long columns), the tile (16 / 8 columns, 32 / 64 at a stride that allows
it, halved to 8, 4 and 2 as n grows), the threads (64 to 512), the one-wave shape of a single radix and whether the twiddle
table lives in LDS or in global memory.  dct_cols_config puts the DCT-II / DCT-III / DST-II / DST-III load and store
(TileCfg::DCT / DST: pairs of real columns) on exactly that configuration; select_jit runs the column pass of a kept-dim plan
(axes.cpp) on it.  test_gpu_dctn.py and test_gpu_dstn.py run columns of 2 to 480 points: the default or a 32-wide tile, the
table in LDS, three passes at most.  Here every class the function can produce gets one length -- the table, its shapes and its
byte counts are tests/test_column_classes_host.py -- and every kernel runs at it against an fp64 reference that does not go
the kernels' route: ref_dct / ref_idct of test_gpu_dct.py (the 4n-point FFT of the even extension), ref_dstn of
test_dst_host.py, numpy.fft.

Every case asserts its class from the plan (the kernel's name with its radices, tile and threads from pass_geometry, the tile
count), writes into a NaN-prefilled output between two NaN guards, finds the guards intact, every element written and its
input bit-identical.  The error is ||got - ref||_2 / ||ref||_2 along the transformed axis for every (batch entry, column)
separately, the worst one bounded by conftest's REL_L2_TOL_F32 / REL_L2_TOL_F64 and nothing else: a norm over a whole entry
would dilute one wrong column of 18 and hide which partner of a pair leaked.  (ref_dstn is the dense sine matrix up to 1080
points, whose own error grows with its arguments: the fp64 sine cases report up to 7e-14 there (1024 points), the
reference's, where the cosine cases report 4e-16.  Beyond 1080 points it is sign, reversal and the cosine reference, held to the matrix in
test_column_classes_host.py.)"""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from test_column_classes_host import BATCH, CLASSES, KEYS, KINDS, ORTHO_KEYS, PRECOMPILED, kept_width, key_id, real_width
from test_dst_host import ref_dstn
from test_gpu_dctn import ref_nd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
TOL = {"f32": REL_L2_TOL_F32, "f64": REL_L2_TOL_F64}
FAR = 1 << 40  # a count at which no grid is clamped by the tile count
GUARD = 64     # NaN elements on both sides of the output

_INPUTS = {}


def _input(tag, t, shape, seed):
    """one input per (family, dtype, shape) and its references by name: computed once, left unchanged"""
    k = (tag, t, shape)
    if k not in _INPUTS:
        x = np.random.default_rng(seed).standard_normal(shape).astype(NP[t])
        x.setflags(write=False)
        _INPUTS[k] = (x, {})
    return _INPUTS[k]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _exec_guarded(plan, x):
    """exec into a NaN-prefilled output with GUARD NaN elements before and behind it, which must stay NaN; x unchanged and
    every output element written"""
    numel = int(np.prod(plan.out_shape))
    keep = x.clone()
    flat = torch.full((GUARD + numel + GUARD,), float("nan"), dtype=plan.out_dtype, device=DEV)
    out = flat[GUARD:GUARD + numel].view(plan.out_shape)
    mf.fft(out, x, plan=plan)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[:GUARD]).all()), "the guard before the output was written"
    assert bool(torch.isnan(flat[GUARD + numel:]).all()), "the guard behind the output was written"
    assert torch.equal(_bits(x), _bits(keep)), "x was written"
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    return out.cpu().numpy()


def _col_err(got, ref):
    """(the worst ||got - ref|| / ||ref|| along axis 1 over every (batch entry, column), its (entry, column)); real or complex
    (b, n, columns)"""
    num = np.linalg.norm(got.astype(ref.dtype) - ref, axis=1)
    den = np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    e = num / den
    where = np.unravel_index(int(e.argmax()), e.shape)
    return float(e.max()), tuple(int(v) for v in where)


def _geo_text(plan, dim):
    geo = plan.pass_geometry(dim)
    return f"{plan.kernel_name(dim)} tile {geo[0]} threads {geo[1]} n_tiles {geo[2]} grid {geo[3]}"


def _assert_class(plan, key, name, columns):
    """pass 0 of the plan is the class the table names for `key`, over `columns` tile columns per batch entry"""
    radices, tile, threads, _ = CLASSES[key]
    text = _geo_text(plan, 0)
    assert plan.kernel_name(0) == name, (text, name)
    assert int(np.prod(plan.stages(0))) == key[1], (text, plan.stages(0))
    assert plan.pass_geometry(0, FAR)[:2] == (tile, threads), (text, tile, threads)
    geo = plan.pass_geometry(0)
    assert geo[2] == BATCH * -(-columns // tile) and 1 <= geo[3] <= geo[2], (text, columns)
    return text


def _name(key, kind=None):
    t, n, _ = key
    return f"cols{n}_" + ("f64_" if t == "f64" else "") + (f"{kind}_" if kind else "") + "x".join(map(str, CLASSES[key][0])) + "_jit"


# ---- pairs of real columns: DCT-II, DCT-III, DST-II, DST-III -----------------------------------------------------------------

PAIRED_CASES = [(k, None) for k in KEYS] + [(k, "ortho") for k in ORTHO_KEYS]


def _paired_id(v):
    return key_id(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key,norm", PAIRED_CASES, ids=_paired_id)
def test_paired_columns(key, norm, kind):
    """(2, n, W) along dim 1: two full tiles of pairs and a ragged one of a single pair (a wide key: two full tiles)"""
    t, n, _ = key
    W = real_width(key)
    shape = (BATCH, n, W, 1)
    inverse, sine = kind.endswith("3"), kind.startswith("dst")
    plan = mf.plan_fft(DT[t], DT[t], shape, shape, inverse=inverse, dctn=True, dst=sine, norm=norm, axes=(1,))
    text = _assert_class(plan, key, _name(key, kind), W // 2)
    assert plan.num_launches == 1 and plan.kernel_name(1) == "none" and plan.scratch_bytes == 0, text
    xh, refs = _input("paired", t, shape[:3], n)
    if (kind, norm) not in refs:
        refs[(kind, norm)] = ref_dstn(xh, (1,), inverse, norm) if sine else ref_nd(xh, (1,), inverse, norm)
    got = _exec_guarded(plan, torch.from_numpy(np.array(xh)).to(DEV).reshape(shape))[..., 0]
    err, where = _col_err(got, refs[(kind, norm)])
    print(f"column-classes paired {kind}{'' if norm is None else '-' + norm} {key_id(key)} W={W}: err {err:.3e} at {where} {text}")
    plan.close()
    assert err <= TOL[t], (key, kind, norm, err, where, text)


# ---- the complex column pass of a kept-dim plan ------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["fft", "ifft"])
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_kept_dim_columns(key, inverse):
    """(2, n, I, 2) along dim 1, the last dim kept: I odd and at least 128 bytes, so that axes.cpp takes a column tile and
    choose_config no wide one (a wide key: I columns, two full tiles).  A length of the precompiled tables takes the
    table's kernel, with its own radices and shape: a column tile it must be; its name and stages are printed (the table's
    column tiles report no geometry through a plan)."""
    t, n, _ = key
    I = kept_width(key)
    shape = (BATCH, n, I, 2)
    plan = mf.plan_fft(DT[t], DT[t], shape, shape, inverse=inverse, axes=(1,))
    assert plan.num_launches == 1 and plan.kernel_name(1) == "none", plan.kernel_name(1)
    if key in PRECOMPILED:
        # (pass_geometry answers for runtime-specialised passes and table rows only: -15 for a table's column tile)
        text = f"{plan.kernel_name(0)} stages {plan.stages(0)} (precompiled: no geometry through the plan)"
        assert plan.kernel_name(0).startswith(f"cols{n}_"), text  # (not "generic", not "ilv")
    else:
        text = _assert_class(plan, key, _name(key), I)
    xh, refs = _input("kept", t, shape, n + 1)
    if inverse not in refs:
        xc = xh[..., 0].astype(np.float64) + 1j * xh[..., 1].astype(np.float64)
        refs[inverse] = (np.fft.ifft if inverse else np.fft.fft)(xc, axis=1)
    out = _exec_guarded(plan, torch.from_numpy(np.array(xh)).to(DEV))
    got = out[..., 0].astype(np.float64) + 1j * out[..., 1].astype(np.float64)
    err, where = _col_err(got, refs[inverse])
    print(f"column-classes kept-dim {'ifft' if inverse else 'fft'} {key_id(key)} I={I}: err {err:.3e} at {where} {text}")
    plan.close()
    assert err <= TOL[t], (key, inverse, err, where, text)


@pytest.mark.parametrize("inverse", [False, True], ids=["fft", "ifft"])
@pytest.mark.parametrize("n", [2080, 4096])
def test_kept_dim_columns_where_the_column_configuration_is_refused(n, inverse):
    """fp64 2080 and 4096: choose_config refuses both (tests/test_column_classes_host.py), the plan must still be right on
    whatever it falls back to; the route is printed"""
    I = 9
    shape = (BATCH, n, I, 2)
    plan = mf.plan_fft(torch.float64, torch.float64, shape, shape, inverse=inverse, axes=(1,))
    xh, refs = _input("kept", "f64", shape, n + 1)
    if inverse not in refs:
        xc = xh[..., 0] + 1j * xh[..., 1]
        refs[inverse] = (np.fft.ifft if inverse else np.fft.fft)(xc, axis=1)
    out = _exec_guarded(plan, torch.from_numpy(np.array(xh)).to(DEV))
    err, where = _col_err(out[..., 0] + 1j * out[..., 1], refs[inverse])
    print(f"column-classes kept-dim {'ifft' if inverse else 'fft'} f64-{n} I={I}: err {err:.3e} at {where} route "
          f"{plan.kernel_name(0)} stages {plan.stages(0)} launches {plan.num_launches} scratch {plan.scratch_bytes}")
    plan.close()
    assert err <= REL_L2_TOL_F64, (n, inverse, err, where)


# ---- a column pass of a new class behind the row pass ------------------------------------------------------------------------

@pytest.mark.parametrize("fn", ["dctn", "dstn"])
@pytest.mark.parametrize("t,n", [("f32", 2401), ("f64", 2025)], ids=["f32-2401", "f64-2025"])
def test_composition_with_the_row_pass(t, n, fn):
    """the full transform of (2, n, 64), both dims: 32 pairs of columns of a tile-2 class, run in place on the rows' result"""
    key = (t, n, None)
    shape = (BATCH, n, 64, 1)
    sine = fn == "dstn"
    kind = "dst2" if sine else "dct2"
    plan = mf.plan_fft(DT[t], DT[t], shape, shape, dctn=True, dst=sine)
    text = _assert_class(plan, key, _name(key, kind), 32)
    assert plan.num_launches == 2 and f"rows64_{'f64_' if t == 'f64' else ''}{kind}_" in plan.kernel_name(1), plan.kernel_name(1)
    xh, refs = _input("both", t, shape[:3], n + 2)
    if fn not in refs:
        refs[fn] = ref_dstn(xh, (1, 2)) if sine else ref_nd(xh, (1, 2))
    got = _exec_guarded(plan, torch.from_numpy(np.array(xh)).to(DEV).reshape(shape))[..., 0]
    ref = refs[fn]
    b = got.shape[0]
    err = float((np.linalg.norm((got - ref).reshape(b, -1), axis=1) / np.linalg.norm(ref.reshape(b, -1), axis=1)).max())
    print(f"column-classes {fn} {t} (2, {n}, 64): err {err:.3e} {text} rows {plan.kernel_name(1)}")
    plan.close()
    assert err <= TOL[t], (t, n, fn, err, text)
