"""The host side of tests/test_gpu_packed_families.py: the pure shape rules that file sizes its cases with, held to the
geometry they promise at every tile the packed rows have; the library's device-free acceptance of every length class by the
families the sweep adds; and the fp64 models the sweep compares the kernels with, evaluated at the sweep's own lengths -- odd
half lengths included, where none of them had run -- against each other, against the direct sum and against torch.autograd
through torch.stft / torch.istft, to the 1e-12 of the existing host tests.  A GPU failure must not be the first time a model
meets such a length.

The batch of a model comparison is the smallest that has every row kind (three rows per channel; one at 2058 points, where the
direct triple sum costs seconds): the batch changes nothing a model computes per row.  Lengths, taps, steps, blocks, windows
and crops are the GPU cases'."""
import types

import numpy as np
import pytest
import torch

import hackathon_fft_amd as mf
import istft_grad_reference as IR
from istft_reference import rel_l2_blocks
from stft_grad_reference import adjoint_model as stft_adjoint_model
from stft_grad_reference import frames_of, torch_stft, window_of
from test_fftconv_grad_host import gk_direct, gk_of, wgrad_model, worst_row
from test_fftconv_host import ref_fftconv
from test_fftconv_long_host import geometry, ols_model
from test_fftconv_part_host import part_geometry, part_model
from test_gpu_packed_lengths import CLASSES, ISTFT_LENGTHS, LENGTHS, SPEC_LENGTHS, _frames, _ids, _stft_shape

DT = {"f32": torch.float32, "f64": torch.float64}
NO_DEVICE = types.SimpleNamespace(device=-1)  # (the checks come first: an accepted request ends in status -10, no device)
ACCEPTED, UNSUPPORTED = -10, -15
HOST_TOL = 1e-12
D = 2           # the channels of every convolution case
CHEAP = 2058    # the longest length at which the direct sums and torch.autograd are run
FP32_SPEC = [tn for tn in SPEC_LENGTHS if tn[0] == "f32"]  # 14, 2058, 10000: one butterfly, a small tile, one row of 512 threads
HALF_LENGTHS = FP32_SPEC + [("f32", 13122)]   # the 16-bit storage cases: and an odd N at 1024 threads
ADJ23_LENGTHS = FP32_SPEC + [("f64", 10240)]  # the `_adj2` / `_adj3` cases: and the longest fp64 frame
assert HALF_LENGTHS[:3] == [("f32", 14), ("f32", 2058), ("f32", 10000)]


# ---- the shape rules, shared with the GPU file ---------------------------------------------------------------------------------

def single_shape(n):
    """(L, K, o, Lo) of a single-block case: L odd and L + K - 1 = n, so the linear result fills the FFT exactly and a wrong
    bin N or a wrap by one sample shows; the window o = 1, Lo = n - 2 starts and ends on an odd sample (real-by-real stores at
    both ends)"""
    L = (n // 2) | 1
    return L, n + 1 - L, 1, n - 2


def full_and_ragged(tile):
    """the fewest work items that are two full tiles and a ragged one (one row per tile: three tiles)"""
    return 2 * tile + max(1, tile // 3)


def blocks_per_row(tile):
    """three blocks per signal row -- four where three would be exactly one tile (tile = 3), so that no tile ever held the
    blocks of two signal rows"""
    return 3 if tile == 1 or 3 % tile else 4


def block_shape(n, taps, tile):
    """(S, F, T) of an overlap-save row under `taps` taps per block: F blocks of S = n - taps + 1 stored samples, the last one
    ragged (a third of a block, one sample at least)"""
    S, F = n - taps + 1, blocks_per_row(tile)
    return S, F, (F - 1) * S + max(1, S // 3)


def block_rows(tile, F, multiple):
    """the fewest signal rows, a multiple of `multiple`, whose rows * F (row, block) pairs are two full tiles and a ragged one"""
    R = -(-full_and_ragged(tile) // F)
    while R % multiple or (tile > 1 and (R * F) % tile == 0):
        R += 1
    return R


def tiles_of(tile, pairs):
    return -(-pairs // tile)


def straddles(tile, F, pairs):
    """some tile of `tile` consecutive (row, block) pairs holds blocks of two signal rows"""
    return any((t * tile) // F != (min((t + 1) * tile, pairs) - 1) // F for t in range(tiles_of(tile, pairs)))


def ols_taps(n):
    return n // 4 + 1


def part_taps(n):
    """(Q, K): three partitions, the last ragged"""
    Q = n // 4 + 1
    return Q, 2 * Q + Q // 2


def istft_geometry(t, n):
    """(tile, threads, where the twiddle table lives) istft_rows_config (csrc/kernels_jit.cpp) makes of the class of (t, n), or
    None where it refuses: tile, table and a carry of N complex elements in 156 KiB keep the table in LDS; tile and carry in
    160 KiB move it to global memory, and a 1024-thread configuration whose table was in LDS drops to 512 threads; else the
    length is refused.  The table has sum over the passes k >= 1 of P_k (R_k - 1) entries (test_gpu_packed_lengths.CLASSES)."""
    radices, tile, threads = CLASSES[(t, n)]
    N, esz = n // 2, 16 if t == "f64" else 8
    table = sum(int(np.prod(radices[:k])) * (radices[k] - 1) for k in range(1, len(radices)))
    was_in_lds = (N * tile + table) * esz <= 156 * 1024
    if (N * tile + table + N) * esz <= 156 * 1024:
        return tile, threads, "lds"
    if (N * tile + N) * esz <= 160 * 1024:
        return tile, 512 if was_in_lds and threads == 1024 else threads, "global"
    return None


def stft_adj_shape(tile, n):
    """(hop, F, T) of a gradient-of-stft case: test_stft's frames (an odd hop, centred by reflection, both edge strips written)"""
    hop = (n // 4) | 1
    F, T = _stft_shape(tile, n, hop)
    return hop, F, T


def istft_adj_shape(tile, n):
    """(hop, F, T) of a gradient-of-istft case: test_istft's frames, `length` one sample short of the covered span"""
    hop, F = n // 4, _frames(tile)
    return hop, F, mf.istft_length(F, n, hop, True) - 1


# ---- the rules give the geometry they promise -------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_the_shape_rules_at_the_tile_of_every_class(tn):
    t, n = tn
    tile = CLASSES[tn][1]
    L, K, o, Lo = single_shape(n)
    assert L % 2 == 1 and L + K - 1 == n and 2 <= L <= n and 1 <= K <= n and o % 2 == 1 and (o + Lo) % 2 == 1 and o + Lo <= n
    # rows of a single block: whole batches of D channels
    R = block_rows(tile, 1, D)
    assert R % D == 0 and R >= 2 * tile + 1 and tiles_of(tile, R) >= 3 and (tile == 1 or R % tile), (tile, R)
    assert R < full_and_ragged(tile) + D + 1  # (no larger than the rule needs)
    # (row, block) pairs of the forward block kernels and of one channel of the filter gradient
    for taps in (ols_taps(n), part_taps(n)[0]):
        S, F, T = block_shape(n, taps, tile)
        assert S >= 1 and F == -(-T // S) and T % S and F in (3, 4)
        for multiple in (D, 1):
            pairs = block_rows(tile, F, multiple) * F
            assert pairs >= 2 * tile + 1 and tiles_of(tile, pairs) >= 3 and (tile == 1 or pairs % tile), (tile, pairs)
            assert tile == 1 or straddles(tile, F, pairs), (tile, F, pairs)
    Q, Kp = part_taps(n)
    assert -(-Kp // Q) == 3 and Kp % Q and 1 <= Q <= n - 1
    B = block_rows(tile, 1, 1)  # the pairs of one channel of the single-block filter gradient
    assert B >= 2 * tile + 1 and tiles_of(tile, B) == 3 and (tile == 1 or B % tile)


def test_three_blocks_never_straddle_a_tile_of_three():
    """why blocks_per_row answers four at tile = 3: with three, every tile is one signal row"""
    assert not any(straddles(3, 3, rows * 3) for rows in range(1, 9)) and straddles(3, 4, block_rows(3, 4, D) * 4)
    assert {blocks_per_row(tile) for _, tile, _ in CLASSES.values() if tile != 3} == {3}


@pytest.mark.parametrize("tn", sorted(set(LENGTHS) | set(ISTFT_LENGTHS)), ids=_ids)
def test_the_framed_shapes(tn):
    t, n = tn
    tile = CLASSES[tn][1]
    if tn in ISTFT_LENGTHS:
        hop, F, T = stft_adj_shape(tile, n)
        assert hop % 2 == 1 and frames_of(T, n, hop, "reflect") == F and T >= n // 2 + 1
        assert F >= 3 and (tile == 1 or (F > tile and F % tile))
        e = min(n // 2, n + hop * (F - 1) - n // 2 - T)
        assert e > 0, "the second edge strip is written too"
    if tn in LENGTHS:
        hop, F, T = istft_adj_shape(tile, n)
        assert F == (tile + 1 if tile > 1 else 3) and 2 * F >= 2 * tile + 1 and T == hop * (F - 1) - 1 >= 1
        assert T - ((F - 1) * hop - n // 2) < n, "the last frame reaches beyond T: it sees a selected zero"


# ---- acceptance without a device -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tn", list(CLASSES), ids=_ids)
def test_every_class_is_a_convolution_length(tn):
    t, n = tn
    assert mf.fftconv_length(n, DT[t]) == n
    assert mf.fftconv_length(n - 1, DT[t]) == n  # (what a user with an odd linear length gets)


def _status(make):
    with pytest.raises(mf.MifftError) as e:
        make()
    return e.value.status, str(e.value)


@pytest.mark.parametrize("tn", LENGTHS, ids=_ids)
def test_the_gradient_planners_accept_every_length(tn):
    t, n = tn
    tile = CLASSES[tn][1]
    L, K, o, Lo = single_shape(n)
    assert _status(lambda: mf.plan_fftconv_grad(DT[t], 3, D, L, n, offset=o, out_length=Lo, partials=1, ctx=NO_DEVICE))[0] == ACCEPTED
    S, F, T = block_shape(n, ols_taps(n), tile)
    assert _status(lambda: mf.plan_fftconv_grad(DT[t], 3, D, T, n, taps=ols_taps(n), partials=1, pregate=True, postgate=True,
                                                ctx=NO_DEVICE))[0] == ACCEPTED
    hop, F, T = istft_adj_shape(tile, n)
    assert _status(lambda: mf.plan_istft_adjoint(DT[t], 2, F, n, hop, window=IR.window_of("hann", n), center=True, length=T,
                                                 ctx=NO_DEVICE))[0] == ACCEPTED  # (fp64 12288 included: no carry beside the tile)


@pytest.mark.parametrize("tn", ISTFT_LENGTHS, ids=_ids)
def test_the_stft_adjoint_planner_and_the_istft_rule(tn):
    t, n = tn
    radices, tile, threads = CLASSES[tn]
    # none of the lengths of the table is a 1024-thread configuration whose table the carry pushes out: tile and threads are
    # the class's; the table moves out at fp64 8192, 9600, 10000 and 10240
    assert istft_geometry(t, n)[:2] == (tile, threads)
    assert (istft_geometry(t, n)[2] == "global") == (tn in (("f64", 8192), ("f64", 9600), ("f64", 10000), ("f64", 10240)))
    hop, F, T = stft_adj_shape(tile, n)
    for mult in (None, 2, 1):
        st, why = _status(lambda: mf.plan_stft_adjoint(DT[t], 2, T, n, hop, window=window_of("hann", n), center="reflect",
                                                       multiplier=mult, ctx=NO_DEVICE))
        assert st == ACCEPTED, (mult, st, why)


def test_the_stft_adjoint_refuses_fp64_12288():
    assert istft_geometry("f64", 12288) is None
    st, why = _status(lambda: mf.plan_stft_adjoint(torch.float64, 2, 12288 * 2, 12288, 3073, center="reflect", ctx=NO_DEVICE))
    assert st == UNSUPPORTED and "carry" in why, (st, why)


# ---- the references agree with each other --------------------------------------------------------------------------------------

def _ns(cheap=False):
    """the distinct (n, tile) of LENGTHS: the models are fp64 whatever the kernel's type, which only sets the tile"""
    seen = sorted({(n, CLASSES[(t, n)][1]) for t, n in LENGTHS})
    return [v for v in seen if not cheap or v[0] <= CHEAP]


def _rows(n):
    return D * (3 if n < CHEAP else 1)


@pytest.mark.parametrize("n,tile", _ns(), ids=str)
@pytest.mark.parametrize("correlate", [False, True])
def test_the_three_forward_models_agree(n, tile, correlate):
    rng = np.random.default_rng(n + tile)
    R = 2 * D
    # the single block is an overlap-save plan of one block, and a partitioned one of one partition
    L, K, o, Lo = single_shape(n)
    x, k = rng.standard_normal((R, L)), rng.standard_normal((D, K))
    one = ref_fftconv(x, k, n, o, Lo, correlate)
    assert worst_row(ols_model(x, k, n, o, Lo, 0, 1, Lo, correlate), one) <= HOST_TOL
    if not correlate:  # ... and, filling the FFT exactly, the linear convolution itself
        lin = np.stack([np.convolve(x[r], k[r % D]) for r in range(R)])
        assert lin.shape[1] == n and worst_row(one, lin[:, o:o + Lo]) <= HOST_TOL
    # the partitioned case's signal and filter through all three: partitions, blocks of all K taps, one long FFT
    Q, Kp = part_taps(n)
    S, F, T = block_shape(n, Q, tile)
    x, k = rng.standard_normal((R, T)), rng.standard_normal((D, Kp))
    m = T + Kp + (T + Kp) % 2  # (an even length that holds the linear result; the reference is numpy's FFT at any length)
    lin = ref_fftconv(x, k, m, 0, T, correlate)
    c, S2, s0, F2, P = part_geometry(n, Q, Kp, 0, T, correlate)
    assert (S2, F2, P) == (S, F, 3)
    part, pairs = part_model(x, k, n, Q, c, S, s0, F, T, correlate)
    assert pairs <= F * P and worst_row(part, lin) <= HOST_TOL
    assert worst_row(ols_model(x, k, n, *geometry(n, Kp, 0, T, correlate), T, correlate), lin) <= HOST_TOL
    # the overlap-save case's own taps and rows
    K = ols_taps(n)
    S, F, T = block_shape(n, K, tile)
    x, k = rng.standard_normal((R, T)), rng.standard_normal((D, K))
    m = T + K + (T + K) % 2
    ols = ols_model(x, k, n, *geometry(n, K, 0, T, correlate), T, correlate)
    assert worst_row(ols, ref_fftconv(x, k, m, 0, T, correlate)) <= HOST_TOL
    assert worst_row(part_model(x, k, n, K, *geometry(n, K, 0, T, correlate), T, correlate)[0], ols) <= HOST_TOL


def _direct(x, gy, K, o, correlate=False):
    """gk_direct's double sum with the sum over t as one numpy dot product per lag: the same terms, no FFT"""
    R, L = x.shape
    t = np.arange(gy.shape[1])
    gk = np.zeros((D, K))
    for r in range(R):
        for j in range(K):
            s = o + t + j if correlate else o + t - j
            ok = (s >= 0) & (s < L)
            gk[r % D, j] += np.dot(gy[r, ok], x[r, s[ok]])
    return gk


def _against_the_direct_sum(n, gk, x, gy, K, o, correlate=False):
    """every lag against the direct sum; gk_direct itself on all K lags where its triple loop is cheap, on the first 16 at
    2058 points (2 x 10^7 terms otherwise) beside its vectorised twin on all of them"""
    want = _direct(x, gy, K, o, correlate)
    Kd = K if n < CHEAP else 16
    assert worst_row(want[:, :Kd], gk_direct(x, gy, D, Kd, o, correlate)) <= HOST_TOL
    assert worst_row(gk, want) <= HOST_TOL, (n, correlate)


@pytest.mark.parametrize("n,tile", _ns(cheap=True), ids=str)
def test_the_filter_gradient_model_against_the_direct_sum(n, tile):
    rng = np.random.default_rng(3 * n + tile)
    R = _rows(n)
    L, K, o, Lo = single_shape(n)
    x, gy = rng.standard_normal((R, L)), rng.standard_normal((R, Lo))
    used = np.zeros((R, Lo), dtype=int)
    A = wgrad_model(x, gy, n, D, o, Lo, 0, 1, Lo, used=used)
    assert (used == 1).all()
    _against_the_direct_sum(n, gk_of(A, n, K), x, gy, K, o)  # (L + K - 1 = n: nothing wraps)
    K = ols_taps(n)
    S, F, T = block_shape(n, K, tile)
    x, gy = rng.standard_normal((R, T)), rng.standard_normal((R, T))
    for correlate in (False, True):
        c, S, s0, F = geometry(n, K, 0, T, correlate)
        used = np.zeros((R, T), dtype=int)
        A = wgrad_model(x, gy, n, D, c, S, s0, F, T, correlate, used=used)
        assert (used == 1).all(), "every sample of gy enters exactly one block"
        _against_the_direct_sum(n, gk_of(A, n, K), x, gy, K, 0, correlate)


def _framed(cheap_lengths):
    return sorted({(n, CLASSES[(t, n)][1]) for t, n in cheap_lengths if n <= CHEAP})


@pytest.mark.parametrize("n,tile", _framed(ISTFT_LENGTHS), ids=str)
def test_the_stft_adjoint_model_against_torch_autograd(n, tile):
    hop, F, T = stft_adj_shape(tile, n)
    B, w = 2, window_of("hann", n)
    g = torch.Generator().manual_seed(n + tile)
    x = torch.randn(B, T, generator=g, dtype=torch.float64, requires_grad=True)
    X = torch_stft(x, n, hop, "reflect", w)
    assert X.shape == (B, n // 2 + 1, F)
    gX = torch.complex(torch.randn(X.shape, generator=g, dtype=torch.float64), torch.randn(X.shape, generator=g, dtype=torch.float64))
    (ref,) = torch.autograd.grad(X, x, gX, retain_graph=True)
    gx, out, edge = stft_adjoint_model(gX.transpose(-1, -2).numpy(), None, 1, w, n, hop, T, "reflect")
    assert rel_l2_blocks(gx, ref.numpy(), hop) <= HOST_TOL
    assert not np.isnan(edge[:, 0]).any() and not np.isnan(edge[:, 1, 0]).any(), "both strips are written"
    Xf = X.detach().transpose(-1, -2).numpy()
    for mode, power in ((2, 2), (3, 1)):
        P = X.abs().pow(power)
        gP = torch.randn(P.shape, generator=g, dtype=torch.float64)
        (ref,) = torch.autograd.grad(P, x, gP, retain_graph=True)
        gx, _, _ = stft_adjoint_model(Xf, gP.transpose(-1, -2).numpy(), mode, w, n, hop, T, "reflect")
        assert rel_l2_blocks(gx, ref.numpy(), hop) <= HOST_TOL, mode


@pytest.mark.parametrize("n,tile", _framed(LENGTHS), ids=str)
def test_the_istft_adjoint_model_against_torch_autograd(n, tile):
    hop, F, T = istft_adj_shape(tile, n)
    shape = (2, F, n, hop, True, "hann", n, T, False)
    X, gy, gX = IR.reference(shape, np.float64, seed=n + tile)
    got = IR.adjoint_model(gy, shape).transpose(0, 2, 1)  # bins-major, as torch's
    err = np.linalg.norm(got - gX, axis=1) / np.linalg.norm(gX, axis=1)
    assert err.max() <= HOST_TOL, err.max()
    N = n // 2
    assert (got[:, 0].imag == 0).all() and (got[:, N].imag == 0).all()
