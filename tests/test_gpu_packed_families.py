"""The sweep of tests/test_gpu_packed_lengths.py -- one row length per configuration CLASS of the packed rows -- through the
kernel families that came to ride on packed_rows_config() after it: the fused convolution (single block, gated overlap-save,
partitioned, 16-bit storage), its filter gradient (plain and gated overlap-save), the gradient of stft / spectrogram
(`_istft_adj1/2/3`), the gradient of istft (`_stft_iadj`) and the sine transforms.  Their own tests run even half lengths,
almost all powers of two: the product stage's pair (k, N - k) with an odd N, the register accumulators of the filter gradient
and of the partitioned kernel at tiles of 62, 42 and 3 rows, and the fp64 adjoints past 1024 points first run here.

The discipline is that file's.  Every case asserts its class from the plan (radices from kernel_name, tile and threads from
pass_geometry, the family's suffix in the name); conv_rows_config and stft_rows_config change neither tile nor threads, the
filter gradient keeps both and has its own n_tiles and grid (tile_launch_geometry), istft_rows_config follows
test_packed_families_host.istft_geometry.  Outputs lie between guards of NaN and start as NaN; inputs come back bit for bit.
Shapes come from the pure rules of test_packed_families_host.py, which holds them to what they promise: two full tiles and
a ragged one of rows or of (row, block) pairs, a tile that holds blocks of two signal rows wherever a tile is more than one
pair (rows of three blocks, the last ragged -- four at tile = 3, where three would be exactly one tile), two entries whose
frames straddle a tile.  References and error measures are the fp64 models of each family's own module, bounded by conftest's
REL_L2_TOL_F32 / REL_L2_TOL_F64, or bit identity for the 16-bit storage; nothing else."""
import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
import istft_grad_reference as IR
from conftest import REL_L2_TOL_F32, REL_L2_TOL_F64
from istft_reference import rel_l2_blocks
from stft_grad_reference import adjoint_model as stft_adjoint_model
from stft_grad_reference import window_of
from test_dst_host import ref_dst2, ref_dst4
from test_fftconv_grad_host import gk_of, wgrad_model, worst_row
from test_fftconv_host import ref_fftconv
from test_fftconv_long_host import geometry, ols_model
from test_fftconv_part_host import model as part_model
from test_gpu_fftconv import _worst
from test_gpu_packed_lengths import CLASSES, DCT_CASES, ISTFT_LENGTHS, LENGTHS, _assert_class, _ids, _report, _run_rows
from test_packed_families_host import (ADJ23_LENGTHS, D, HALF_LENGTHS, block_rows, block_shape, istft_adj_shape, istft_geometry,
                                       ols_taps, part_taps, single_shape, stft_adj_shape, straddles, tiles_of)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
TOL = {"f32": REL_L2_TOL_F32, "f64": REL_L2_TOL_F64}
HALF = {"b16": torch.bfloat16, "h16": torch.float16}
FAR = 1 << 40  # a count at which no grid is clamped by the tile count
GUARD = 64     # NaN elements on both sides of every output


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _between(shape, dtype):
    """a NaN-prefilled tensor of `shape` in the middle of a buffer of NaN: (whole, view)"""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def _guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def _launch(call, outs, ins):
    """call() between a snapshot of the inputs' bits and the checks every case makes: the guards of every output still NaN,
    every input bit for bit what it was"""
    keep = [_bits(v).clone() for v in ins]
    call()
    torch.cuda.synchronize()
    for flat in outs:
        assert _guards_intact(flat), "a guard beside an output was written"
    for v, k in zip(ins, keep):
        assert torch.equal(_bits(v), k), "an input was written"


def _normal(seed, shape, dtype):
    """standard-normal values rounded to `dtype` on the device, and the same values in float64 on the host"""
    v = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).to(dtype)
    return v.to(DEV), v.double().numpy()


def _conv(plan, x, a=None, b=None):
    """the exec of a convolution plan, gated or not -> out (rows, Lo, 1), wholly written"""
    flat, out = _between(plan.out_shape, x.dtype)
    if plan.conv_gates:
        _launch(lambda: plan.run(out, x, pregate=a, postgate=b), [flat], [x, a, b])
    else:
        _launch(lambda: mf.fft(out, x, plan=plan), [flat], [x])
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    return out


def _wgrad(plan, x, gy, a=None, b=None):
    """the exec of a filter-gradient plan -> out (P, D, n / 2 + 1, 2), wholly written"""
    flat, out = _between(plan.out_shape, plan.out_dtype)
    kw = {k: v for k, v in (("pregate", a), ("postgate", b)) if v is not None}
    _launch(lambda: plan.run(out, x, gy, **kw), [flat], [v for v in (x, gy, a, b) if v is not None])
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    return out


def _cplx(out):
    o = out.cpu().numpy().astype(np.float64)
    return o[..., 0] + 1j * o[..., 1]


def _block_class(plan, t, n, suffix, tile, F, rows):
    """the class, the suffix and the tiles of a forward block kernel over `rows` signal rows of F blocks"""
    text = _assert_class(plan, 1, t, n, threads_too=True)  # (conv_rows_config: tile and threads are the packed rows')
    geo = plan.pass_geometry(1)
    assert plan.kernel_name(1).endswith(suffix + "_jit") and plan.kernel_name(0) == "none" and plan.num_launches == 1, text
    assert plan.blocks == F and geo[2] == tiles_of(tile, rows * F) >= 3 and (tile == 1 or (rows * F) % tile), (text, rows, F)
    assert tile == 1 or straddles(tile, F, rows * F), text
    return text


# ---- 1. the single block ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_conv_single_block(tn):
    t, n = tn
    L, K, o, Lo = single_shape(n)
    make = lambda B: mf.plan_fftconv(DT[t], B, D, L, n, offset=o, out_length=Lo)
    tile = make(1).pass_geometry(1, FAR)[0]
    R = block_rows(tile, 1, D)
    plan = make(R // D)
    text = _block_class(plan, t, n, "_conv", tile, 1, R)
    x, xh = _normal(n, (R, L, 1), DT[t])
    k, kh = _normal(n + 1, (D, K), DT[t])
    plan.set_filter(k)
    got = _conv(plan, x).cpu().numpy()[..., 0]
    err = _worst(got, ref_fftconv(xh[..., 0], kh, n, o, Lo))
    _report("conv", t, n, err, f"{text} rows={R} L={L} K={K} o={o} Lo={Lo}")
    assert err <= TOL[t], (t, n, err, text)


# ---- 2. gated overlap-save ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_conv_overlap_save_gated(tn):
    t, n = tn
    K, correlate = ols_taps(n), LENGTHS.index(tn) % 2 == 1
    make = lambda B, T: mf.plan_fftconv(DT[t], B, D, T, n, taps=K, correlate=correlate, pregate=True, postgate=True)
    tile = make(1, block_shape(n, K, 1)[2]).pass_geometry(1, FAR)[0]
    S, F, T = block_shape(n, K, tile)
    R = block_rows(tile, F, D)
    plan = make(R // D, T)
    text = _block_class(plan, t, n, "_conv_ols_g3", tile, F, R)
    assert plan.step == S
    x, xh = _normal(n, (R, T, 1), DT[t])
    a, ah = _normal(n + 1, (R, T, 1), DT[t])
    b, bh = _normal(n + 2, (R, T, 1), DT[t])
    k, kh = _normal(n + 3, (D, K), DT[t])
    plan.set_filter(k)
    got = _conv(plan, x, a, b).cpu().numpy()[..., 0]
    ref = ols_model((ah * xh)[..., 0], kh, n, *geometry(n, K, 0, T, correlate), T, correlate) * bh[..., 0]
    err = _worst(got, ref)
    _report("conv_ols_g3", t, n, err, f"{text} rows={R} T={T} K={K} S={S} F={F} correlate={correlate}")
    assert err <= TOL[t], (t, n, err, text)


# ---- 3. partitioned ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_conv_partitioned(tn):
    t, n = tn
    Q, K = part_taps(n)
    make = lambda B, T: mf.plan_fftconv(DT[t], B, D, T, n, taps=K, partition=Q)
    tile = make(1, block_shape(n, Q, 1)[2]).pass_geometry(1, FAR)[0]
    S, F, T = block_shape(n, Q, tile)
    R = block_rows(tile, F, D)
    plan = make(R // D, T)
    text = _block_class(plan, t, n, "_conv_pols", tile, F, R)
    assert (plan.step, plan.partitions) == (S, 3)
    x, xh = _normal(n, (R, T, 1), DT[t])
    k, kh = _normal(n + 3, (D, K), DT[t])
    plan.set_filter(k)
    got = _conv(plan, x).cpu().numpy()[..., 0]
    err = _worst(got, part_model(xh[..., 0], kh, n, Q, 0, T))
    _report("conv_pols", t, n, err, f"{text} rows={R} T={T} K={K} Q={Q} S={S} F={F}")
    assert err <= TOL[t], (t, n, err, text)


# ---- 4. the filter gradient ---------------------------------------------------------------------------------------------------

def _wgrad_class(plan, t, n, suffix, tile, pairs):
    """tile and threads are the packed rows'; n_tiles and grid are the filter gradient's own (tile_launch_geometry,
    csrc/kernels_jit.cpp): one workgroup per (channel, partial), each walking ceil(its pairs / tile) steps"""
    text = _assert_class(plan, 1, t, n, threads_too=True)
    geo = plan.pass_geometry(1)
    assert plan.kernel_name(1).endswith(suffix + "_jit") and plan.kernel_name(0) == "none" and plan.num_launches == 1, text
    assert plan.partials == 1 and geo[3] == D and geo[2] == D * tiles_of(tile, pairs) and tiles_of(tile, pairs) >= 3, (text, pairs)
    assert tile == 1 or pairs % tile, (text, pairs)
    return text


@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_wgrad_single_block(tn):
    t, n = tn
    L, K, o, Lo = single_shape(n)
    make = lambda B: mf.plan_fftconv_grad(DT[t], B, D, L, n, offset=o, out_length=Lo, partials=1)
    tile = make(1).pass_geometry(1)[0]
    B = block_rows(tile, 1, 1)  # (the pairs of ONE channel are what a workgroup walks)
    plan = make(B)
    text = _wgrad_class(plan, t, n, "_wgrad", tile, B)
    x, xh = _normal(n, (B * D, L, 1), DT[t])
    gy, gh = _normal(n + 1, (B * D, Lo, 1), DT[t])
    A = _cplx(_wgrad(plan, x, gy))
    want = wgrad_model(xh[..., 0], gh[..., 0], n, D, o, Lo, 0, 1, Lo)
    err = worst_row(A, want)  # every row of bins
    gk = plan.filter_grad(x, gy, K)
    err_k = worst_row(gk.cpu().numpy(), gk_of(want, n, K))
    _report("wgrad", t, n, err, f"gk err {err_k:.3e} {text} pairs per channel={B} L={L} K={K} o={o} Lo={Lo}")
    assert err <= TOL[t] and err_k <= TOL[t], (t, n, err, err_k, text)


@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_wgrad_overlap_save_gated(tn):
    t, n = tn
    K, correlate = ols_taps(n), LENGTHS.index(tn) % 2 == 0
    make = lambda B, T: mf.plan_fftconv_grad(DT[t], B, D, T, n, taps=K, correlate=correlate, partials=1, pregate=True, postgate=True)
    tile = make(1, block_shape(n, K, 1)[2]).pass_geometry(1)[0]
    S, F, T = block_shape(n, K, tile)
    B = block_rows(tile, F, 1)
    plan = make(B, T)
    text = _wgrad_class(plan, t, n, "_wgrad_ols_g3", tile, B * F)
    assert (plan.blocks, plan.step) == (F, S) and (tile == 1 or straddles(tile, F, B * F)), text
    x, xh = _normal(n, (B * D, T, 1), DT[t])
    a, ah = _normal(n + 1, (B * D, T, 1), DT[t])
    gy, gh = _normal(n + 2, (B * D, T, 1), DT[t])
    b, bh = _normal(n + 3, (B * D, T, 1), DT[t])
    A = _cplx(_wgrad(plan, x, gy, a, b))
    want = wgrad_model((ah * xh)[..., 0], (bh * gh)[..., 0], n, D, *geometry(n, K, 0, T, correlate), T, correlate)
    err = worst_row(A, want)
    gk = plan.filter_grad(x, gy, K, pregate=a, postgate=b)
    err_k = worst_row(gk.cpu().numpy(), gk_of(want, n, K))
    _report("wgrad_ols_g3", t, n, err, f"gk err {err_k:.3e} {text} pairs per channel={B * F} T={T} K={K} S={S} F={F} correlate={correlate}")
    assert err <= TOL[t] and err_k <= TOL[t], (t, n, err, err_k, text)


# ---- 5. 16-bit storage: the float32 kernel's bits ------------------------------------------------------------------------------

HALF_CASES = [(tn, "b16") for tn in HALF_LENGTHS] + [(("f32", 2058), "h16")]


@pytest.mark.parametrize("tn,ts", HALF_CASES, ids=_ids)
def test_conv_half_storage(tn, ts):
    """the gated single block on 16-bit rows: the float32 kernel on the widened tensors, rounded once to the storage type"""
    t, n = tn
    io = HALF[ts]
    L, K, o, Lo = single_shape(n)
    make = lambda B, io_dtype: mf.plan_fftconv(DT[t], B, D, L, n, offset=o, out_length=Lo, pregate=True, postgate=True, io_dtype=io_dtype)
    tile = make(1, io).pass_geometry(1, FAR)[0]
    R = block_rows(tile, 1, D)
    hp, fp = make(R // D, io), make(R // D, None)
    text = _block_class(hp, t, n, f"_conv_g3_{ts}", tile, 1, R)
    assert fp.kernel_name(1) == hp.kernel_name(1).replace(f"_{ts}", "") and fp.pass_geometry(1) == hp.pass_geometry(1), text
    x, a, b = (_normal(n + i, shape, io)[0] for i, shape in enumerate(((R, L, 1), (R, L, 1), (R, Lo, 1))))
    k = _normal(n + 3, (D, K), torch.float32)[0]
    hp.set_filter(k)
    fp.set_filter(k)
    got, want = _conv(hp, x, a, b), _conv(fp, x.float(), a.float(), b.float()).to(io)
    bad = int((_bits(got) != _bits(want)).sum())
    _report(f"conv_g3_{ts}", t, n, bad / got.numel(), f"{text} rows={R} L={L} K={K}: {bad} of {got.numel()} samples differ")
    assert got.dtype == io and bad == 0, (t, n, ts, bad, text)


@pytest.mark.parametrize("tn,ts", HALF_CASES, ids=_ids)
def test_wgrad_half_storage(tn, ts):
    """the gated filter gradient of 16-bit rows: the float32 gated kernel's result on the widened tensors, which stays float32"""
    t, n = tn
    io = HALF[ts]
    L, K, o, Lo = single_shape(n)
    make = lambda B, io_dtype: mf.plan_fftconv_grad(DT[t], B, D, L, n, offset=o, out_length=Lo, partials=1, pregate=True, postgate=True,
                                                    io_dtype=io_dtype)
    tile = make(1, io).pass_geometry(1)[0]
    B = block_rows(tile, 1, 1)
    hp, fp = make(B, io), make(B, None)
    text = _wgrad_class(hp, t, n, f"_wgrad_g3_{ts}", tile, B)
    assert fp.kernel_name(1) == hp.kernel_name(1).replace(f"_{ts}", "") and fp.pass_geometry(1) == hp.pass_geometry(1), text
    x, a, gy, b = (_normal(n + i, shape, io)[0] for i, shape in enumerate(((B * D, L, 1), (B * D, L, 1), (B * D, Lo, 1), (B * D, Lo, 1))))
    got, want = _wgrad(hp, x, gy, a, b), _wgrad(fp, x.float(), gy.float(), a.float(), b.float())
    bad = int((_bits(got) != _bits(want)).sum())
    _report(f"wgrad_g3_{ts}", t, n, bad / got.numel(), f"{text} pairs per channel={B}: {bad} of {got.numel()} words differ")
    assert got.dtype == torch.float32 and bad == 0, (t, n, ts, bad, text)


# ---- 6. the gradient of stft / spectrogram --------------------------------------------------------------------------------------

ADJ_CASES = [(tn, 1) for tn in ISTFT_LENGTHS] + [(tn, mode) for mode in (2, 3) for tn in ADJ23_LENGTHS]


@pytest.mark.parametrize("tn,mode", ADJ_CASES, ids=_ids)
def test_stft_adjoint(tn, mode):
    """periodic Hann, an odd hop, centred by reflection: out and both edge strips against the fp64 model of the launch, NaN
    exactly where the model writes nothing, and the folded gradient in the block measure of test_gpu_stft_grad.py"""
    t, n = tn
    mult, w = {1: None, 2: 2, 3: 1}[mode], window_of("hann", n)
    make = lambda B, T, hop: mf.plan_stft_adjoint(DT[t], B, T, n, hop, window=w, center="reflect", multiplier=mult)
    probe = make(1, n, (n // 4) | 1)
    tile = probe.pass_geometry(2, FAR)[0]
    probe.close()
    hop, F, T = stft_adj_shape(tile, n)
    B, N = 2, n // 2
    plan = make(B, T, hop)
    # istft_rows_config may move the twiddle table out and drop 1024 threads to 512; at no length of the table does it (the
    # rule is istft_geometry, held to this by test_packed_families_host.py): tile and threads are the class's
    assert istft_geometry(t, n)[:2] == CLASSES[tn][1:]
    text = _assert_class(plan, 2, t, n, threads_too=True)
    assert plan.kernel_name(2).endswith(f"_istft_adj{mode}_jit") and plan.kernel_name(1) == "none" and plan.num_launches == 1, text
    assert plan.frames == F and plan.pass_geometry(2)[2] == B * tiles_of(tile, F) and (tile == 1 or F % tile), text
    g, gh = _normal(n + mode, (B, F, N + 1, 2), DT[t])
    m, mh = _normal(n + 7, (B, F, N + 1), DT[t])
    of, out = _between(plan.out_shape, DT[t])
    ef, edge = _between(plan.edge_shape, DT[t])
    ins = [g] + ([m] if mult is not None else [])
    _launch(lambda: plan.run(out, g, multiplier=m if mult is not None else None, edge=edge), [of, ef], ins)
    gx, out_m, edge_m = stft_adjoint_model(gh[..., 0] + 1j * gh[..., 1], mh, mode, w, n, hop, T, "reflect")
    got, strips = out.cpu().numpy()[..., 0].astype(np.float64), edge.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(out_m)) and np.array_equal(np.isnan(strips), np.isnan(edge_m)), text
    e = int((~np.isnan(edge_m[0, 1])).sum())
    assert plan.covered == T and e > 0, "every sample and both strips are written"
    got[:, 1:N + 1] += strips[:, 0, ::-1]  # the fold of StftAdjointPlan.apply
    got[:, T - 1 - e:T - 1] += strips[:, 1, :e][:, ::-1]
    err = rel_l2_blocks(got, gx, hop)
    _report(f"istft_adj{mode}", t, n, err, f"{text} B={B} T={T} F={F} hop={hop}")
    plan.close()
    assert err <= TOL[t], (t, n, mode, err, text)


# ---- 7. the gradient of istft ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_istft_adjoint(tn):
    """periodic Hann, hop n // 4, centred, `length` one sample short of the covered span: the last frame of every entry sees a
    selected zero.  Every length of the table is accepted (fp64 12288 too: the STFT tile keeps no carry; the host file asserts
    the library's answer).  The worst frame's relative l2 against the fp64 model, as test_gpu_istft_grad.py measures it."""
    t, n = tn
    w = IR.window_of("hann", n)
    make = lambda B, F, T: mf.plan_istft_adjoint(DT[t], B, F, n, n // 4, window=w, center=True, length=T)
    probe = make(1, 3, None)
    tile = probe.pass_geometry(1, FAR)[0]
    probe.close()
    hop, F, T = istft_adj_shape(tile, n)
    B, N = 2, n // 2
    plan = make(B, F, T)
    text = _assert_class(plan, 1, t, n, threads_too=True)  # (stft_rows_config: tile and threads are the packed rows')
    assert plan.kernel_name(1).endswith("_stft_iadj_jit") and plan.num_launches == 1 and plan.scratch_bytes == 0, text
    assert plan.pass_geometry(1)[2] == tiles_of(tile, B * F) >= 3 and (tile == 1 or F % tile), text
    gy, gh = _normal(n + 5, (B, T, 1), DT[t])
    flat, out = _between(plan.out_shape, DT[t])
    _launch(lambda: mf.fft(out, gy, plan=plan), [flat], [gy])
    assert not bool(torch.isnan(out).any()), "a part of the output was not written"
    ref = IR.adjoint_model(gh[..., 0], (B, F, n, hop, True, "hann", n, T, False))
    got = _cplx(out)
    den = np.linalg.norm(ref, axis=-1)
    assert (den > 0).all()
    err = float((np.linalg.norm(got - ref, axis=-1) / den).max())
    _report("stft_iadj", t, n, err, f"{text} B={B} F={F} hop={hop} T={T}")
    im = _bits(out[..., 1])
    assert int(im[..., 0].abs().max()) == 0 and int(im[..., N].abs().max()) == 0, (text, "Im of bins 0 / n/2 is not +0")
    plan.close()
    assert err <= TOL[t], (t, n, err, text)


# ---- 8. the sine transforms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dst2", "dst3", "dst4"])
@pytest.mark.parametrize("tn,norm", DCT_CASES, ids=_ids)
def test_dst_rows(tn, norm, kind):
    t, n = tn
    make = lambda b: mf.plan_fft(DT[t], DT[t], (b, n, 1), (b, n, 1), inverse=kind == "dst3", dct=True, dst=True, norm=norm,
                                 dct_type=4 if kind == "dst4" else 2)
    ref = {"dst2": lambda x: ref_dst2(x[..., 0], norm), "dst3": lambda x: ref_dst2(x[..., 0], norm, True),
           "dst4": lambda x: ref_dst4(x[..., 0], norm)}[kind]
    _run_rows(kind, t, n, make, lambda b: (b, n, 1), ref, norm)
