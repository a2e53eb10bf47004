"""Host-side mirror of the reference's GPU call surface, over the libmifft C ABI.

Reference interface (fft/fft/fft.mojo):
    plan_fft[in_dtype, out_dtype, in_layout, out_layout, *, bases, inverse,
             runtime_twfs, max_cluster_size, _test](*, ctx) -> _GPUPlan   (:161-210)
    fft(output, x, ctx, *, plan)                                          (:262-323)
Mojo's compile-time parameters become ordinary arguments here; layouts are
shapes ``(batch, d0[, d1[, d2]], C)`` of row-major tensors.

PyTorch is used only as the owner of device memory and streams: tensors are
handed to the library as raw device pointers.  Nothing in this module computes
an FFT on the host or through torch.fft.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import enum
import functools
import hashlib
import math
import threading
from fractions import Fraction
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import MifftError, check

# mifft_dtype (include/mifft.h).  Input tensors may have any of these element types -- the reference casts in its
# first-stage load (fft/fft/_fft.mojo:243-257); the output is float32 or float64.
_DTYPE_CODE = {torch.float32: 0, torch.float64: 1, torch.uint8: 2, torch.int32: 3, torch.int8: 4, torch.int16: 5,
               torch.float16: 7, torch.bfloat16: 8}
if hasattr(torch, "uint16"):
    _DTYPE_CODE[torch.uint16] = 6
_OUT_DTYPES = (torch.float32, torch.float64)
_IO_DTYPES = (torch.bfloat16, torch.float16)  # the 16-bit storage types of a convolution plan (io_dtype; float32 inside)

FLAG_FAITHFUL_STAGES = 1
FLAG_HALF_SPECTRUM = 2  # MIFFT_FLAG_HALF_SPECTRUM: numpy's one-sided rfftn / irfftn layouts (include/mifft.h)
FLAG_DCT = 4            # MIFFT_FLAG_DCT: DCT-II (inverse: its inverse) of real rows, (batch, n, 1) on both sides
FLAG_DCT_ORTHO = 8      # MIFFT_FLAG_DCT_ORTHO: scipy's norm="ortho" of such a plan
FLAG_DCT_ND = 16        # MIFFT_FLAG_DCT_ND: N-D DCT-II (inverse: its inverse) of real tensors, (batch, d0.., 1) on both sides
FLAG_STFT = 32                 # MIFFT_FLAG_STFT: framed, windowed real signals, (batch, T, 1) -> (batch, F, n // 2 + 1, 2)
FLAG_STFT_CENTER_REFLECT = 64  # MIFFT_FLAG_STFT_CENTER_REFLECT: frames centred, the signal reflected at both ends
FLAG_STFT_CENTER_ZEROS = 128   # MIFFT_FLAG_STFT_CENTER_ZEROS: frames centred, zeros beyond both ends
FLAG_STFT_HOP_MASK = 0xFFFF0000
FLAG_ISTFT = 0x4000            # MIFFT_FLAG_ISTFT: overlap-added frames, (batch, F, n // 2 + 1, 2) -> (batch, T, 1); hop and centre bits shared
FLAG_STFT_POWER = 0x8000       # MIFFT_FLAG_STFT_POWER: beside FLAG_STFT, real |X| ** power or its filterbanked bands instead of X
STFT_EXT_TAG_LO = 0x46465401   # MIFFT_STFT_EXT_TAG_LO / _HI: the NaN in the power slot that selects the extended payload of such
STFT_EXT_TAG_HI = 0x7FF84D49   # a plan (log stage, matrix after the bands)
STFT_MAX_BANDS = 32768         # MIFFT_STFT_MAX_BANDS
DCT_TYPE4_TAG = 0x44435434     # MIFFT_DCT_TYPE4_TAG: the first ``bases`` word of a FLAG_DCT plan that is a DCT-IV
DST_TAG = 0x44535432           # MIFFT_DST_TAG: the first ``bases`` word of a FLAG_DCT / FLAG_DCT_ND plan that is a DST-II
DST_TYPE4_TAG = 0x44535434     # MIFFT_DST_TYPE4_TAG: the first ``bases`` word of a FLAG_DCT plan that is a DST-IV
MDCT_TAG_LO = 0x43544401       # MIFFT_MDCT_TAG_LO / _HI: the NaN behind the window of a FLAG_STFT plan that is an MDCT
MDCT_TAG_HI = 0x7FF84D44
CONV_TAG_LO = 0x4F4E5601       # MIFFT_CONV_TAG_LO / _HI: the NaN in front of the 8-word payload of a FLAG_STFT plan that is a
CONV_TAG_HI = 0x7FF84D43       # fused FFT convolution (TAG | D | o | Lo | mode | the device address of the filter spectra)
GATED_ARGS_MAGIC = 0x314147544646494D  # MIFFT_GATED_ARGS_MAGIC ("MIFFTGA1")
CONV_GRAD_TAG_LO = 0x44524701  # MIFFT_CONV_GRAD_TAG_LO / _HI: the NaN in front of the 16-word payload of a FLAG_STFT plan that is the
CONV_GRAD_TAG_HI = 0x7FF84D47  # filter gradient of a fused convolution (TAG | D | c | S | mode | F | s0 | Lo | P | 0 | gates | 0 x 4)
CONV_GRAD_ARGS_MAGIC = 0x314757544646494D  # MIFFT_CONV_GRAD_ARGS_MAGIC ("MIFFTWG1")
CONV_GRAD_GATED_ARGS_MAGIC = 0x324757544646494D  # MIFFT_CONV_GRAD_GATED_ARGS_MAGIC ("MIFFTWG2")
CONV_PAIR_TAG_LO = 0x49415001  # MIFFT_CONV_PAIR_TAG_LO / _HI: the NaN in front of the 16-word payload of a FLAG_STFT plan that is the
CONV_PAIR_TAG_HI = 0x7FF84D50  # convolution of two signal batches (TAG | K | ea | eb | o | Lo | mode | 0 x 8)
CONV_PAIR_ARGS_MAGIC = 0x314150544646494D  # MIFFT_CONV_PAIR_ARGS_MAGIC ("MIFFTPA1")
STFT_ADJ_TAG_LO = 0x4A444101   # MIFFT_STFT_ADJ_TAG_LO / _HI: the NaN behind the window of a FLAG_ISTFT plan that is the adjoint of
STFT_ADJ_TAG_HI = 0x7FF84D41   # the STFT (w | TAG | gain | mode, 0)
ISTFT_ADJ_TAG_LO = 0x4A444901  # MIFFT_ISTFT_ADJ_TAG_LO / _HI: the NaN behind the window of a FLAG_STFT plan that is the adjoint of
ISTFT_ADJ_TAG_HI = 0x7FF84D4A  # the inverse STFT (w | TAG | gain | frames, 0)
STFT_ADJ_ARGS_MAGIC = 0x314153544646494D  # MIFFT_STFT_ADJ_ARGS_MAGIC ("MIFFTSA1")
MAX_DIMS = 6            # MIFFT_MAX_DIMS


class GatedArgs(ctypes.Structure):
    """mifft_gated_args: what the exec of a gated convolution plan takes, by host address, in the place of x"""
    _fields_ = [("magic", ctypes.c_uint64), ("x", ctypes.c_void_p), ("pregate", ctypes.c_void_p),
                ("postgate", ctypes.c_void_p)]


class ConvGradArgs(ctypes.Structure):
    """mifft_conv_grad_args: what the exec of a filter-gradient plan takes, by host address, in the place of x"""
    _fields_ = [("magic", ctypes.c_uint64), ("x", ctypes.c_void_p), ("gy", ctypes.c_void_p)]


class ConvGradGatedArgs(ctypes.Structure):
    """mifft_conv_grad_gated_args: what the exec of a filter-gradient plan with gates takes, by host address, in the place of x"""
    _fields_ = [("magic", ctypes.c_uint64), ("x", ctypes.c_void_p), ("gy", ctypes.c_void_p), ("pregate", ctypes.c_void_p),
                ("postgate", ctypes.c_void_p)]


class ConvPairArgs(ctypes.Structure):
    """mifft_conv_pair_args (include/mifft.h): the argument block of a two-signal convolution exec"""
    _fields_ = [("magic", ctypes.c_uint64), ("x", ctypes.c_void_p), ("v", ctypes.c_void_p)]


class StftAdjArgs(ctypes.Structure):
    """mifft_stft_adj_args: what the exec of an STFT adjoint plan takes, by host address, in the place of x"""
    _fields_ = [("magic", ctypes.c_uint64), ("x", ctypes.c_void_p), ("mult", ctypes.c_void_p), ("edge", ctypes.c_void_p)]


def FLAG_KEEP_DIM(d: int) -> int:
    """MIFFT_FLAG_KEEP_DIM(d): dim d (0 = the first after the batch) is carried through untransformed"""
    return 1 << (8 + int(d))


FLAG_KEEP_MASK = 0x3F00


def FLAG_STFT_HOP(h: int) -> int:
    """MIFFT_FLAG_STFT_HOP(h): the hop of an STFT plan, 1 .. 65535 samples"""
    h = int(h)
    if not 1 <= h <= 65535:
        raise MifftError(ERR_UNSUPPORTED, f"the hop of an STFT plan is 1 .. 65535 samples, got {h}")
    return h << 16


ERR_UNSUPPORTED = -15   # MIFFT_ERR_UNSUPPORTED


class GPUTest(enum.Enum):
    """The reference's code-path forcing knob (_GPUTest, fft/fft/_ndim_fft_gpu.mojo:453-459).

    CDNA4 has no thread-block clusters and one synchronisation scope that matters
    (the workgroup), so every value selects the same thing here: the literal
    stage-per-pass kernel family instead of the fused register-butterfly kernels.
    """
    BLOCK = 0
    WARP = 1
    DEVICE_WIDE = 2
    CLUSTER = 3


class DeviceContext:
    """Stand-in for Mojo's DeviceContext: a device plus the stream work is enqueued on."""

    def __init__(self, device: Optional[int] = None, stream: Optional["torch.cuda.Stream"] = None):
        if not torch.cuda.is_available():
            raise MifftError(-10, "no HIP device visible to torch; libmifft has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._stream = stream

    @property
    def stream(self) -> "torch.cuda.Stream":
        return self._stream if self._stream is not None else torch.cuda.current_stream(self.device)

    def synchronize(self) -> None:
        self.stream.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def ordered_bases(length: int, bases: Sequence[int]) -> list:
    """Descending per-stage radices (_get_ordered_bases_processed_list, fft/fft/_utils.mojo:186-221)."""
    n = len(bases)
    arr = (ctypes.c_uint32 * max(n, 1))(*[int(b) for b in bases])
    out = (ctypes.c_uint32 * 64)()
    k = check(_lib.lib().mifft_ordered_bases(int(length), arr, n, out, 64))
    return list(out[:k])


def estimate_best_bases(length: int, target: str = "gpu") -> list:
    """_estimate_best_bases (fft/fft/fft.mojo:49-104)."""
    out = (ctypes.c_uint32 * 64)()
    k = check(_lib.lib().mifft_estimate_bases(int(length), 1 if target == "gpu" else 0, out, 64))
    return list(out[:k])


def estimate_best_bases_nd(in_shape: Sequence[int], out_shape: Sequence[int], target: str = "gpu") -> list:
    """_estimate_best_bases_nd (fft/fft/fft.mojo:107-119)."""
    _check_layout_conditions_nd(tuple(in_shape), tuple(out_shape))
    return [estimate_best_bases(d, target) for d in out_shape[1:-1]]


def _check_layout_conditions_nd(in_shape: tuple, out_shape: tuple) -> None:
    """_check_layout_conditions_nd (fft/fft/fft.mojo:20-46), raised at plan time instead of compile time."""
    rank = len(out_shape)
    if rank <= 2:
        raise MifftError(-1, "The rank should be bigger than 2. The first dimension represents the amount of "
                             "batches, and the last the complex dimension.")
    if len(in_shape) != rank:
        raise MifftError(-1, "in_layout and out_layout must have equal rank")
    if not 1 <= in_shape[-1] <= 2:
        raise MifftError(-3, "The last dimension of in_layout should be 1 or 2")
    if out_shape[-1] != 2:
        raise MifftError(-3, "out_layout must have the last dimension equal to 2")
    if tuple(out_shape[:-1]) != tuple(in_shape[:-1]):
        raise MifftError(-2, "out_layout and in_layout should have the same shape before the last dimension")
    for i in range(rank - 2):
        if out_shape[i + 1] == 1:
            raise MifftError(-2, "no inner dimension should be of size 1")


def _check_half_layout(in_shape: tuple, out_shape: tuple, inverse: bool) -> tuple:
    """Layouts of a half-spectrum plan (MIFFT_FLAG_HALF_SPECTRUM); returns the logical real dims d0..d{k-1}.
    forward: x (batch, d0.., n, 1) -> out (batch, d0.., n // 2 + 1, 2); inverse: the other way round."""
    rank = len(out_shape)
    if rank <= 2 or len(in_shape) != rank:
        raise MifftError(-1, "half-spectrum layouts are (batch, d0[, d1..], C) with equal ranks")
    real, cplx = (out_shape, in_shape) if inverse else (in_shape, out_shape)
    if real[-1] != 1:
        raise MifftError(-3, f"the real side of a half-spectrum plan has 1 component, got {real[-1]}")
    if cplx[-1] != 2:
        raise MifftError(-3, f"the half-spectrum side of a plan has 2 components, got {cplx[-1]}")
    dims = real[1:-1]
    if any(d == 1 for d in dims):
        raise MifftError(-2, "no inner dimension should be of size 1")
    n = dims[-1]
    if n % 2:
        raise MifftError(ERR_UNSUPPORTED, f"half spectrum of an odd last dimension ({n}) is not supported")
    if tuple(cplx[:-2]) != tuple(real[:-2]) or cplx[-2] != n // 2 + 1:
        raise MifftError(-2, f"half-spectrum side {cplx} does not match the real side {real}: the last dimension "
                             f"holds n // 2 + 1 = {n // 2 + 1} bins")
    return dims


def _check_dct_layout(in_shape: tuple, out_shape: tuple) -> tuple:
    """Layouts of a DCT plan (MIFFT_FLAG_DCT): both sides real rows (batch, n, 1) of one shape; returns the dims (n,)."""
    if len(in_shape) != 3 or len(out_shape) != 3:
        raise MifftError(-2, f"DCT layouts are (batch, n, 1) on both sides, got {in_shape} -> {out_shape}")
    if in_shape[-1] != 1 or out_shape[-1] != 1:
        raise MifftError(-3, f"both sides of a DCT plan have 1 component, got {in_shape[-1]} and {out_shape[-1]}")
    if in_shape != out_shape:
        raise MifftError(-2, f"a DCT writes as many reals as it reads: {in_shape} -> {out_shape}")
    n = in_shape[1]
    if n % 2 or n < 8:
        raise MifftError(ERR_UNSUPPORTED, f"DCT of an odd length or of fewer than 8 points ({n}) is not supported")
    return (n,)


def _check_dctn_layout(in_shape: tuple, out_shape: tuple) -> tuple:
    """Layouts of an N-D DCT plan (MIFFT_FLAG_DCT_ND): both sides real (batch, d0.., 1) of one shape; returns the dims d0.."""
    if len(in_shape) < 3 or len(in_shape) != len(out_shape):
        raise MifftError(-1, f"N-D DCT layouts are (batch, d0[, d1..], 1) with equal ranks, got {in_shape} -> {out_shape}")
    if len(in_shape) - 2 > MAX_DIMS:
        raise MifftError(-1, f"at most {MAX_DIMS} dims between batch and the trailing 1, got {len(in_shape) - 2}")
    if in_shape[-1] != 1 or out_shape[-1] != 1:
        raise MifftError(-3, f"both sides of a DCT plan have 1 component, got {in_shape[-1]} and {out_shape[-1]}")
    if in_shape != out_shape:
        raise MifftError(-2, f"a DCT writes as many reals as it reads: {in_shape} -> {out_shape}")
    dims = in_shape[1:-1]
    if any(d == 1 for d in dims):
        raise MifftError(-2, "no inner dimension should be of size 1")
    return dims


_STFT_CENTER_FLAGS = {None: 0, "reflect": FLAG_STFT_CENTER_REFLECT, "constant": FLAG_STFT_CENTER_ZEROS}


def _stft_center_flags(center) -> int:
    """``center`` of an STFT plan as flag bits: None (frames start at multiples of the hop), "reflect" or "constant" """
    if center is not None and not isinstance(center, str) or center not in _STFT_CENTER_FLAGS:
        raise MifftError(ERR_UNSUPPORTED, f"center must be None, \"reflect\" or \"constant\", got {center!r}")
    return _STFT_CENTER_FLAGS[center]


def stft_frames(length: int, n_fft: int, hop_length: int, center=False) -> int:
    """Frames torch.stft makes of ``length`` samples: 1 + (length - n_fft) // hop_length, centred (any true ``center``: the
    signal is extended by n_fft // 2 at both ends) 1 + length // hop_length.  Pure host arithmetic."""
    length, n_fft, hop_length = int(length), int(n_fft), int(hop_length)
    if hop_length < 1:
        raise MifftError(ERR_UNSUPPORTED, f"hop_length must be positive, got {hop_length}")
    if center:
        return 1 + length // hop_length
    if length < n_fft:
        raise MifftError(ERR_UNSUPPORTED, f"a signal of {length} samples is shorter than one frame of {n_fft}")
    return 1 + (length - n_fft) // hop_length


def _check_stft_layout(in_shape: tuple, out_shape: tuple, hop: int, center) -> tuple:
    """Layouts of an STFT plan (MIFFT_FLAG_STFT): x (batch, T, 1) real -> out (batch, F, n // 2 + 1, 2) with
    F = stft_frames(T, n, hop, center); returns the dims (T, n), n = 2 (out_shape[2] - 1)."""
    if len(in_shape) != 3 or len(out_shape) != 4:
        raise MifftError(-1, f"STFT layouts are (batch, T, 1) -> (batch, F, n // 2 + 1, 2), got {in_shape} -> {out_shape}")
    if in_shape[-1] != 1:
        raise MifftError(-3, f"an STFT reads real signals (1 component), got {in_shape[-1]}")
    if out_shape[-1] != 2:
        raise MifftError(-3, f"an STFT writes complex bins (2 components), got {out_shape[-1]}")
    if in_shape[0] != out_shape[0]:
        raise MifftError(-2, f"batch {in_shape[0]} of x against {out_shape[0]} of out")
    T, n = in_shape[1], 2 * (out_shape[2] - 1)
    if n < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with frames of fewer than 8 points ({n}) is not supported")
    FLAG_STFT_HOP(hop)
    mode = _stft_center_flags(center)
    if T < 2:
        raise MifftError(-2, f"signals of {T} samples: at least 2")
    if mode == FLAG_STFT_CENTER_REFLECT and n // 2 > T - 1:
        raise MifftError(ERR_UNSUPPORTED, f"center=\"reflect\" needs n_fft // 2 <= T - 1 (one reflection), got n_fft = {n}, "
                                          f"T = {T}")
    frames = stft_frames(T, n, hop, mode != 0)
    if out_shape[1] != frames:
        raise MifftError(-2, f"{T} samples in frames of {n} every {hop} make {frames} frames, out has {out_shape[1]}")
    return (T, n)


def _spec_power(power) -> int:
    """``power`` of a spectrogram plan: 1 (magnitude) or 2 (power)"""
    if isinstance(power, bool) or not isinstance(power, (int, float)) or power not in (1, 2):
        raise MifftError(ERR_UNSUPPORTED, f"power must be 1 (magnitude) or 2 (power), got {power!r}")
    return int(power)


def _fb_f64(fb, bins: Optional[int] = None) -> "torch.Tensor":
    """a filterbank as a (bins, M) float64 matrix on the host (a CUDA tensor is copied, which synchronises its stream)"""
    t = torch.as_tensor(fb)
    if t.is_complex():
        raise MifftError(-3, "the filterbank must be real")
    t = t.detach().to(device="cpu", dtype=torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] < 1 or (bins is not None and t.shape[0] != bins):
        want = "n_fft // 2 + 1" if bins is None else str(bins)
        raise MifftError(-2, f"the filterbank is {tuple(t.shape)}, expected ({want}, M): one row per bin, one column per band "
                             f"(a librosa-style (M, bins) matrix must be transposed)")
    return t


def _f64_words(values) -> list:
    """float64 values as they travel through ``bases`` (window_words, for long tables)"""
    import numpy as np
    a = torch.as_tensor(values).detach().to(device="cpu", dtype=torch.float64).contiguous().numpy()
    return np.frombuffer(a.tobytes(), dtype="<u4").tolist()


def _check_spec_layout(in_shape: tuple, out_shape: tuple, hop: int, center, fb, post=None) -> tuple:
    """Layouts of a spectrogram plan (MIFFT_FLAG_STFT | MIFFT_FLAG_STFT_POWER): x (batch, T, 1) real -> out
    (batch, F, n // 2 + 1, 1) real, or (batch, F, M, 1) with a filterbank ``fb`` of shape (n // 2 + 1, M), or (batch, F, Q, 1)
    with an (M, Q) matrix ``post`` after it; returns the dims (T, n)."""
    if len(out_shape) != 4:
        raise MifftError(-1, f"spectrogram layouts are (batch, T, 1) -> (batch, F, n // 2 + 1 or M, 1), got {in_shape} -> "
                             f"{out_shape}")
    if out_shape[-1] != 1:
        raise MifftError(-3, f"a spectrogram plan writes real values (1 component), got {out_shape[-1]}")
    bins = out_shape[2]
    if fb is not None:
        bins = int(fb.shape[0])
        if post is not None:
            if out_shape[2] != post.shape[1]:
                raise MifftError(-2, f"a matrix post of {tuple(post.shape)} makes {post.shape[1]} values, out has {out_shape[2]}")
        elif out_shape[2] != fb.shape[1]:
            raise MifftError(-2, f"a filterbank of {tuple(fb.shape)} makes {fb.shape[1]} bands, out has {out_shape[2]}")
    return _check_stft_layout(in_shape, out_shape[:2] + (bins, 2), hop, center)


def _spec_log(log, what: str = "stft_log") -> tuple:
    """the log stage of a spectrogram plan as four floats (add, amin, a, c): y = a * log2(max(v + add, amin)) + c"""
    import math
    try:
        vals = tuple(float(v) for v in log)
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 4:
        raise MifftError(ERR_UNSUPPORTED, f"{what} is (add, amin, a, c), four numbers, got {log!r}")
    add, amin, a, c = vals
    if not math.isfinite(add) or add < 0:
        raise MifftError(-5, f"add (eps) of the log stage is finite and not negative, got {add!r}")
    if not (amin > 0 and math.isfinite(amin)):
        raise MifftError(-5, f"amin of the log stage is positive and finite, got {amin!r}")
    if not math.isfinite(a) or a == 0:
        raise MifftError(-5, f"a of the log stage is finite and not zero, got {a!r}")
    if not math.isfinite(c):
        raise MifftError(-5, f"c of the log stage is finite, got {c!r}")
    return vals


def _post_f64(post, bands: Optional[int]) -> "torch.Tensor":
    """the matrix after the bands as an (M, Q) float64 matrix on the host (a CUDA tensor is copied, which synchronises)"""
    t = torch.as_tensor(post)
    if t.is_complex():
        raise MifftError(-3, "post must be real")
    t = t.detach().to(device="cpu", dtype=torch.float64).contiguous()
    if bands is None:
        raise MifftError(ERR_UNSUPPORTED, "post without fb: the matrix applies to the bands of a filterbank")
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[0] != bands:
        raise MifftError(-2, f"post is {tuple(t.shape)}, expected ({bands}, Q): one row per band of the filterbank, one column "
                             f"per output")
    if t.shape[1] > STFT_MAX_BANDS:
        raise MifftError(-9, f"post has {t.shape[1]} columns: at most {STFT_MAX_BANDS}")
    return t


_LOG_KINDS = ("log", "log10", "db")


def _log_stage(log, amin, eps, ref, power: int) -> Optional[tuple]:
    """``log`` / ``amin`` / ``eps`` / ``ref`` of plan_spectrogram and spectrogram as the (add, amin, a, c) of the plan"""
    import math
    if log is None:
        if ref != 1.0:
            raise MifftError(ERR_UNSUPPORTED, "ref without log=\"db\"")
        return None
    if not isinstance(log, str) or log not in _LOG_KINDS:
        raise MifftError(ERR_UNSUPPORTED, f"log must be None, \"log\", \"log10\" or \"db\", got {log!r}")
    try:
        amin, eps, ref = float(amin), float(eps), float(ref)
    except (TypeError, ValueError):
        raise MifftError(ERR_UNSUPPORTED, f"amin, eps and ref are numbers, got {amin!r}, {eps!r}, {ref!r}") from None
    if log != "db":
        if ref != 1.0:
            raise MifftError(ERR_UNSUPPORTED, f"ref belongs to log=\"db\", not to log={log!r}")
        return _spec_log((eps, amin, math.log(2.0) if log == "log" else math.log10(2.0), 0.0), "log")
    if not (ref > 0 and math.isfinite(ref)):
        raise MifftError(-5, f"ref of log=\"db\" is positive and finite, got {ref!r}")
    if not (amin > 0 and math.isfinite(amin)):
        raise MifftError(-5, f"amin of the log stage is positive and finite, got {amin!r}")
    mult = 10.0 if power == 2 else 20.0
    return _spec_log((eps, amin, mult * math.log10(2.0), -mult * math.log10(max(amin, ref))), "log")


def istft_length(frames: int, n_fft: int, hop_length: int, center=False) -> int:
    """Samples torch.istft returns by default for ``frames`` frames: n_fft + hop_length * (frames - 1), less n_fft // 2 at both
    ends when centred.  Pure host arithmetic."""
    frames, n_fft, hop_length = int(frames), int(n_fft), int(hop_length)
    if hop_length < 1:
        raise MifftError(ERR_UNSUPPORTED, f"hop_length must be positive, got {hop_length}")
    if frames < 1:
        raise MifftError(-2, f"at least one frame, got {frames}")
    return n_fft + hop_length * (frames - 1) - (2 * (n_fft // 2) if center else 0)


def _istft_center_flags(center) -> int:
    """``center`` of an inverse STFT plan as flag bits: None / False (uncentred), True / "reflect" or "constant" (centred: the
    two bits mean the same here, the first and last n // 2 samples are trimmed)"""
    if center is None or center is False:
        return 0
    if center is True:
        return FLAG_STFT_CENTER_REFLECT
    return _stft_center_flags(center)


def _check_frames_to_signal(what: str, in_shape: tuple, out_shape: tuple, hop: int) -> tuple:
    """what the layouts of an inverse STFT plan and of an STFT adjoint plan (``what``) share: x (batch, F, n // 2 + 1, 2) -> out
    (batch, T, 1) real; returns (T, F, n), n = 2 (in_shape[2] - 1)"""
    if len(in_shape) != 4 or len(out_shape) != 3:
        raise MifftError(-1, f"{what} layouts are (batch, F, n // 2 + 1, 2) -> (batch, T, 1), got {in_shape} -> {out_shape}")
    if in_shape[-1] != 2:
        raise MifftError(-3, f"an {what} reads complex bins (2 components), got {in_shape[-1]}")
    if out_shape[-1] != 1:
        raise MifftError(-3, f"an {what} writes real signals (1 component), got {out_shape[-1]}")
    if in_shape[0] != out_shape[0]:
        raise MifftError(-2, f"batch {in_shape[0]} of x against {out_shape[0]} of out")
    n = 2 * (in_shape[2] - 1)
    if n < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with frames of fewer than 8 points ({n}) is not supported")
    FLAG_STFT_HOP(hop)
    return out_shape[1], in_shape[1], n


def _check_istft_layout(in_shape: tuple, out_shape: tuple, hop: int, center) -> tuple:
    """Layouts of an inverse STFT plan (MIFFT_FLAG_ISTFT): x (batch, F, n // 2 + 1, 2) -> out (batch, T, 1) real with
    2 <= T <= n + hop (F - 1) - (centred: n // 2); returns the dims (T, F, n), n = 2 (in_shape[2] - 1)."""
    T, F, n = _check_frames_to_signal("inverse STFT", in_shape, out_shape, hop)
    if hop > n:
        raise MifftError(ERR_UNSUPPORTED, f"hop_length {hop} > n_fft {n}: gaps between the frames")
    centred = _istft_center_flags(center) != 0
    if F < 1:
        raise MifftError(-2, f"at least one frame, got {F}")
    covered = n + hop * (F - 1) - (n // 2 if centred else 0)
    if not 2 <= T <= covered:
        raise MifftError(-2, f"{F} frames of {n} every {hop} cover 2 .. {covered} output samples, out has {T} "
                             f"(a longer output is not zero-padded)")
    return (T, F, n)


def _check_stft_adjoint_layout(in_shape: tuple, out_shape: tuple, hop: int, center) -> tuple:
    """Layouts of an STFT adjoint plan (MIFFT_STFT_ADJ_TAG on MIFFT_FLAG_ISTFT): x (batch, F, n // 2 + 1, 2) -> out
    (batch, T, 1) real, T the signal's length and F = stft_frames(T, n, hop, center) the forward's frames; returns the dims
    (T, F, n).  ``center`` is the forward plan's: None, "reflect" or "constant"."""
    T, F, n = _check_frames_to_signal("STFT adjoint", in_shape, out_shape, hop)
    if hop > n:
        raise MifftError(ERR_UNSUPPORTED, f"the STFT adjoint with hop_length {hop} > n_fft {n} is not supported: the overlap-add "
                                          f"kernel it runs on has no gaps between its frames")
    if F != stft_frames(T, n, hop, _stft_center_flags(center) != 0):
        raise MifftError(-2, f"signals of {T} samples have {stft_frames(T, n, hop, _stft_center_flags(center) != 0)} frames of "
                             f"{n} every {hop}, x has {F}")
    if center == "reflect" and n // 2 > T - 1:
        raise MifftError(-2, f"reflect padding needs n_fft // 2 <= T - 1, got n_fft = {n}, T = {T}")
    return (T, F, n)


def _check_istft_adjoint_layout(in_shape: tuple, out_shape: tuple, hop: int, center) -> tuple:
    """Layouts of an inverse STFT adjoint plan (MIFFT_ISTFT_ADJ_TAG on MIFFT_FLAG_STFT): x (batch, T, 1) real, the incoming
    gradient -> out (batch, F, n // 2 + 1, 2), with the limits of the inverse plan it is the adjoint of, hop <= n and
    2 <= T <= n + hop (F - 1) - (centred: n // 2), the bound ``_check_istft_layout`` sets for that plan (the C ABI itself
    accepts T = 1 for both); returns the dims (T, n).  ``center``: None / False, or True / "constant"."""
    if len(in_shape) != 3 or len(out_shape) != 4:
        raise MifftError(-1, f"inverse STFT adjoint layouts are (batch, T, 1) -> (batch, F, n // 2 + 1, 2), got {in_shape} -> "
                             f"{out_shape}")
    if center == "reflect":
        raise MifftError(ERR_UNSUPPORTED, "the inverse STFT adjoint sees zeros beyond both ends: center is None / False, True or "
                                          "\"constant\", not \"reflect\"")
    if in_shape[-1] != 1:
        raise MifftError(-3, f"an inverse STFT adjoint reads real gradients (1 component), got {in_shape[-1]}")
    _check_istft_layout(out_shape, in_shape, hop, center)
    return (in_shape[1], 2 * (out_shape[2] - 1))


def _window_f64(window, n_fft: int) -> "torch.Tensor":
    """a window as n_fft float64 values on the host (a CUDA tensor is copied, which synchronises its stream)"""
    w = torch.as_tensor(window).detach().to(device="cpu", dtype=torch.float64).contiguous()
    if w.dim() != 1 or w.numel() != n_fft:
        raise MifftError(-5, f"the window has {tuple(w.shape)} values, the frames {n_fft}")
    return w


def window_words(window) -> list:
    """The window of an STFT plan as it travels through ``bases``: the IEEE binary64 bits of every value as two 32-bit words,
    low word first (include/mifft.h, MIFFT_FLAG_STFT)."""
    raw = torch.as_tensor(window).detach().to(device="cpu", dtype=torch.float64).contiguous().numpy().tobytes()
    return [int.from_bytes(raw[i:i + 4], "little") for i in range(0, len(raw), 4)]


def words_window(words) -> list:
    """the inverse of window_words: the float64 values of a word list"""
    words = [int(v) for v in words]
    raw = b"".join((words[i] | (words[i + 1] << 32)).to_bytes(8, "little") for i in range(0, len(words), 2))
    return (ctypes.c_double * (len(words) // 2)).from_buffer_copy(raw)[:]


class FrameRequest(NamedTuple):
    """What a framed plan that is no convolution is asked for (``ConvRequest`` is the convolutions'): frames of ``n`` samples
    every ``hop``, a ``window`` of n values taken by value (float64 on the host; None: rectangular, the sine window
    mdct_window(hop) for the MDCT pair).  None of the kinds has a reference counterpart.  ``kind``:
    "stft" (``Plan(stft_hop=)``, plan_stft; MIFFT_FLAG_STFT in include/mifft.h, _check_stft_layout): x (batch, T, 1) real ->
        out (batch, F, n // 2 + 1, 2); ``center`` None / "reflect" / "constant".  Payload: w, or nothing without a window.
    "spec" (``stft_power=`` beside it, plan_spectrogram; MIFFT_FLAG_STFT_POWER, _check_spec_layout): the same plan stores
        abs(X) ** ``power`` (1 or 2), real, out (batch, F, n // 2 + 1, 1) -- or, with ``fb`` of shape (n // 2 + 1, M), the M bands
        fb.T @ abs(X) ** power per frame, out (batch, F, M, 1).  Payload: w | power | fb, the window written out.  With ``log``
        (add, amin, a, c) every value v becomes a * log2(max(v + add, amin)) + c first, and with ``post``, an (M, Q) matrix beside
        ``fb``, the plan stores post.T @ (the bands, after the log stage), out (batch, F, Q, 1); either one makes the payload
        w | MIFFT_STFT_EXT_TAG | power, M, Q, log?, add, amin, a, c | fb | post.
    "istft" (``istft_hop=``, plan_istft; MIFFT_FLAG_ISTFT, _check_istft_layout): x (batch, F, n // 2 + 1, 2) -> out (batch, T, 1)
        real; ``center`` None / False or True / "reflect" / "constant" (centred: n // 2 samples trimmed at both ends); ``gain`` a
        factor on the synthesis window that stays out of the envelope.  Payload: w | gain, the gain only when it is not 1,
        nothing without either.
    "adjoint" (``stft_adjoint=`` beside ``istft_hop``, plan_stft_adjoint; MIFFT_STFT_ADJ_TAG, _check_stft_adjoint_layout): the
        adjoint of the "stft" plan of these values, ``adjoint`` its mode 1, 2 or 3.  Payload: w | TAG | gain | mode, 0.
    "istft_adjoint" (``istft_adjoint=`` F beside ``stft_hop``, plan_istft_adjoint; MIFFT_ISTFT_ADJ_TAG on a MIFFT_FLAG_STFT plan,
        _check_istft_adjoint_layout): the adjoint of the "istft" plan of these values and ``frames`` = F frames: x (batch, T, 1),
        the incoming gradient -> out (batch, F, n // 2 + 1, 2); ``center`` None / False or True / "constant"; ``gain`` the
        inverse plan's.  Payload: w | TAG | gain | frames, 0, the window written out.
    "mdct" (``mdct=`` M, plan_mdct; MIFFT_MDCT_TAG, _check_mdct_layout): x (batch, T, 1) -> out (batch, F, M, 1), frames of
        n = 2 M samples every hop = M; ``gain`` the factor on the cosine sum.  Payload: w | TAG | gain.
    "imdct" (``imdct=`` M, plan_imdct; MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan, _check_imdct_layout): x (batch, F, M, 1) ->
        out (batch, T, 1) with 2 <= T <= (F - 1) M; ``gain`` the factor on the synthesis window.  Payload: w | TAG | gain.
    ``bases`` of a forward kind ("stft", "spec", "mdct") has two lists, of an inverse kind three: empty ones and, last, the
    radices of n (MDCT pair: of M // 2), or an empty one for the default.  ``inverse=True`` is implied by the inverse kinds."""
    kind: str
    n: int
    hop: int
    center: object = None
    window: object = None
    gain: float = 1.0
    power: object = None
    fb: object = None
    log: object = None
    post: object = None
    adjoint: int = 0
    frames: int = 0


def _frame_payload(r) -> tuple:
    """(flag bits, payload words, leading lists of ``bases`` that carry no radices) of a ``FrameRequest`` or ``ConvRequest``:
    the one place that knows the word layouts (include/mifft.h).  Pure: no device, no library call; status -5 for a window of
    another length than the frames."""
    if isinstance(r, ConvRequest):
        return FLAG_STFT, _conv_payload(r), 1
    if isinstance(r, ConvPairRequest):
        return FLAG_STFT, _conv_pair_payload(r), 1
    if r.kind not in ("stft", "spec", "istft", "adjoint", "istft_adjoint", "mdct", "imdct"):
        raise MifftError(ERR_UNSUPPORTED, f"unknown kind of framed plan {r.kind!r}")
    bits = FLAG_STFT_HOP(r.hop)
    if r.window is not None:
        w = _f64_words(_window_f64(r.window, r.n))
    elif r.kind == "stft" or (r.kind == "istft" and float(r.gain) == 1.0):
        w = []
    else:  # (every other layout has words behind the window: it is written out)
        w = _f64_words(mdct_window(r.hop) if r.kind in ("mdct", "imdct") else torch.ones(r.n, dtype=torch.float64))
    if r.kind in ("mdct", "imdct"):
        scale = _f64_words(torch.tensor([float(r.gain)], dtype=torch.float64))
        side = (FLAG_STFT, 1) if r.kind == "mdct" else (FLAG_ISTFT, 2)
        return bits | side[0] | FLAG_STFT_CENTER_ZEROS, w + [MDCT_TAG_LO, MDCT_TAG_HI] + scale, side[1]
    if r.kind == "istft":  # (a list of Python floats goes through torch's default dtype: this gain has always travelled as float32's)
        return bits | FLAG_ISTFT | _istft_center_flags(r.center), w + (_f64_words([float(r.gain)]) if float(r.gain) != 1.0 else []), 2
    if r.kind == "istft_adjoint":  # (the gain travels as the inverse plan's does: both plans scale by the same number)
        if r.center == "reflect" or not 1 <= int(r.frames) < 1 << 32:
            raise MifftError(ERR_UNSUPPORTED if r.center == "reflect" else -2,
                             f"an inverse STFT adjoint has center None / False, True or \"constant\" and 1 <= frames < 2^32, got "
                             f"{r.center!r} and {r.frames}")
        centred = FLAG_STFT_CENTER_ZEROS if _istft_center_flags(r.center) else 0
        return (bits | FLAG_STFT | centred,
                w + [ISTFT_ADJ_TAG_LO, ISTFT_ADJ_TAG_HI] + _f64_words([float(r.gain)]) + [int(r.frames), 0], 1)
    bits |= _stft_center_flags(r.center)
    if r.kind == "adjoint":
        return bits | FLAG_ISTFT, w + [STFT_ADJ_TAG_LO, STFT_ADJ_TAG_HI] + _f64_words([float(r.gain)]) + [int(r.adjoint), 0], 2
    if r.kind == "stft":
        return bits | FLAG_STFT, w, 1
    if r.log is None and r.post is None:
        w = w + _f64_words([float(r.power)])
    else:
        head = [float(r.power), 0.0 if r.fb is None else float(r.fb.shape[1]), 0.0 if r.post is None else float(r.post.shape[1]),
                0.0 if r.log is None else 1.0] + list(r.log or (0.0, 0.0, 0.0, 0.0))
        w = w + [STFT_EXT_TAG_LO, STFT_EXT_TAG_HI] + _f64_words(torch.tensor(head, dtype=torch.float64))
    for table in (r.fb, r.post):  # (row by row)
        if table is not None:
            w = w + _f64_words(table)
    return bits | FLAG_STFT | FLAG_STFT_POWER, w, 1


def _pack_bases(words: list, bases, lead: int) -> tuple:
    """``bases`` as the (flat words, list lengths) of mifft_plan_create_slab, (None, None) for the defaults.  A framed plan
    (``lead`` > 0) sends its payload as the first list, empty lists up to ``lead`` and the radices of the last dim."""
    if lead and (words or bases is not None):
        if bases is not None and any(len(bs) for bs in bases[:lead]):
            raise MifftError(-5, "dims 0 and 1 of an inverse STFT plan are not transformed: their bases lists must be empty"
                             if lead == 2 else "dim 0 of an STFT plan is framed, not transformed: its bases list must be empty")
        radices = [int(b) for b in bases[lead]] if bases is not None else []
        flat, lens = words + radices, [len(words)] + [0] * (lead - 1) + [len(radices)]
    elif bases is not None:
        flat, lens = [int(b) for bs in bases for b in bs], [len(bs) for bs in bases]
    else:
        return None, None
    return (ctypes.c_uint32 * max(len(flat), 1))(*flat), (ctypes.c_int32 * len(lens))(*lens)


def _dct_norm_flags(norm) -> int:
    """scipy's ``norm`` of a DCT plan as flag bits: None / "backward" (the unnormalised forward) or "ortho" """
    if norm is None or norm == "backward":
        return 0
    if norm == "ortho":
        return FLAG_DCT_ORTHO
    raise MifftError(ERR_UNSUPPORTED, f"norm must be None, \"backward\" or \"ortho\", got {norm!r}")


def _keep_flags(rank: int, axes) -> int:
    """keep bits (MIFFT_FLAG_KEEP_DIM) of the layout positions 1 .. rank - 2 NOT in ``axes`` (None: every one transformed)"""
    if axes is None:
        return 0
    ax = [int(a) for a in axes]
    for a in ax:
        if not 1 <= a <= rank - 2:
            raise MifftError(-2, f"axes are layout positions 1 .. {rank - 2} (the dims between batch and C), got {a}")
    if len(set(ax)) != len(ax):
        raise MifftError(-2, f"repeated axis in {tuple(ax)}")
    return sum(FLAG_KEEP_DIM(p - 1) for p in range(1, rank - 1) if p not in ax)


_FRAMED_NO_AXES = {"stft": "an STFT plan frames dim 0 and transforms dim 1: no axes",
                   "istft": "an inverse STFT plan transforms dim 2 and overlap-adds dim 1: no axes",
                   "mdct": "an MDCT plan frames dim 0 and transforms dim 1: no axes",
                   "imdct": "an IMDCT plan transforms dim 2 and overlap-adds dim 1: no axes",
                   "conv": "a convolution plan extends dim 0 and transforms dim 1: no axes"}
_FRAMED_NO_AXES.update(spec=_FRAMED_NO_AXES["stft"], adjoint=_FRAMED_NO_AXES["istft"], istft_adjoint=_FRAMED_NO_AXES["stft"])


class Plan:
    """_GPUPlan (fft/fft/_ndim_fft_gpu.mojo:153-207): owns the device twiddle tables.

    ``half_spectrum=True`` (no reference counterpart): numpy's one-sided layouts, see _check_half_layout.
    ``axes`` (no reference counterpart): the layout positions (1 .. rank - 2) to transform; the others are carried through
    untransformed (MIFFT_FLAG_KEEP_DIM).  None: all of them.  With ``bases``, a kept dim's list is empty.
    ``dct=True`` (no reference counterpart): DCT-II of real rows, ``inverse`` its inverse, both sides (batch, n, 1); ``norm``
    is scipy's (None / "backward" / "ortho").  ``bases`` of such a plan holds one list whose radices multiply to n // 2, the
    packed transform the plan runs and ``stages(0)`` reports -- not to n.  See _check_dct_layout and MIFFT_FLAG_DCT in
    include/mifft.h.
    ``dctn=True`` (no reference counterpart): the N-D DCT-II (``inverse``: its inverse) over the dims of a real
    (batch, d0.., 1) tensor, ``axes`` and ``norm`` as above (MIFFT_FLAG_DCT_ND in include/mifft.h, _check_dctn_layout);
    ``bases`` factor n // 2 for a transformed last dim and n for the others.
    ``stft_hop`` > 0 (with ``stft_power`` the spectrogram), ``istft_hop`` > 0 (with ``stft_adjoint`` the STFT's adjoint),
    ``mdct`` = M > 0, ``imdct`` = M > 0: the framed plans, whose keywords ``stft_center``, ``stft_window``, ``stft_fb``,
    ``stft_log``, ``stft_post``, ``istft_gain``, ``mdct_scale`` and ``imdct_gain`` become the fields of a ``FrameRequest``: see
    there for each kind's layouts, payload and ``bases``.  MIFFT_FLAG_STFT or MIFFT_FLAG_ISTFT with a hop in ``flags`` is the
    same request as ``stft_hop`` / ``istft_hop``.
    ``dct_type=4`` beside ``dct=True`` (no reference counterpart): the DCT-IV instead, both directions the same kernel with
    another scale, in_dtype == out_dtype; the request travels as MIFFT_DCT_TYPE4_TAG in front of the radices of n // 2.
    ``dst=True`` beside ``dct=True`` or ``dctn=True`` (no reference counterpart): the sine transform of the same type on the
    same passes (scipy's dst / idst of ``dct_type`` 2 or 4, dstn / idstn of type 2); the request travels as MIFFT_DST_TAG or
    MIFFT_DST_TYPE4_TAG in front of the radices of the first list, and an empty list of such a plan is that dim's default.
    ``conv`` = a ``ConvRequest`` (no reference counterpart): the fused FFT convolution of real rows,
    x (batch, L, 1) -> out (batch, Lo, 1), samples o .. o + Lo - 1 of irfft(rfft(x, n) * G[row % D], n) against the D filter
    spectra at the device ``address`` (mode bit 0: their conjugates); the caller keeps that buffer alive (MIFFT_CONV_TAG in
    include/mifft.h, plan_fftconv).  ``bases`` has two lists, an empty one and the radices of n (or an empty one).
    With ``S`` > 0 it is the overlap-save form: x (batch, T, 1) with T possibly beyond n, ``F`` blocks of n samples per row,
    block f from sample ``s0`` + f S on, of whose circular result the S samples from ``o`` (= c) on are stored at f S of the
    row's Lo output samples; with ``Q`` > 0 besides, partitioned overlap-save in ``P`` partitions of Q taps
    (plan_fftconv(partition=)).  ``gates`` = 1, 2 or 3 on any form: bit 0 a pregate of x's shape multiplied into the load, bit 1
    a postgate of out's shape multiplied into the store; the gates are arguments of every exec (ConvPlan.run).  Bits 8..15 of
    ``mode`` are the storage type of the rows (0, or the code of float16 / bfloat16 under float32: ``ConvPlan.io_dtype``).
    ``grad`` makes it the request of that convolution's filter gradient (``partials``; MIFFT_CONV_GRAD_TAG, ConvGradPlan),
    whose ``out_shape`` is the incoming gradient's.  ``_conv_payload`` is the words of either; ``_frame_payload`` encodes every
    framed request.  ``conv`` = a ``ConvPairRequest`` instead: the convolution of two signal batches (MIFFT_CONV_PAIR_TAG,
    plan_fftconv_pair), x (batch, L, 1) -> out (batch, Lo, 1) with v (batch, K, 1) given beside x at every exec."""

    io_dtype = None  # (a convolution plan with 16-bit rows in memory: ConvPlan / ConvGradPlan; None on every other plan)

    def __init__(self, in_dtype, out_dtype, in_shape, out_shape, *, bases=None, inverse=False,
                 device: int = 0, flags: int = 0, whole_batch: int = 0, half_spectrum: bool = False, axes=None,
                 dct: bool = False, norm=None, dctn: bool = False, stft_hop: int = 0, stft_center=None, stft_window=None,
                 istft_hop: int = 0, istft_gain: float = 1.0, stft_power=None, stft_fb=None, stft_log=None,
                 stft_post=None, dct_type: int = 2, mdct: int = 0, mdct_scale: float = 1.0, imdct: int = 0,
                 imdct_gain: float = 1.0, dst: bool = False, conv=None, stft_adjoint: int = 0,
                 istft_adjoint: int = 0):
        in_shape, out_shape = tuple(int(v) for v in in_shape), tuple(int(v) for v in out_shape)
        mdct, imdct, flags = int(mdct), int(imdct), int(flags)
        if dct_type not in (2, 4):
            raise MifftError(ERR_UNSUPPORTED, f"dct_type must be 2 or 4, got {dct_type!r}")
        stft = not mdct and conv is None and (int(stft_hop) != 0 or bool(flags & FLAG_STFT))  # (the flag bit is the same request)
        istft = int(istft_hop) != 0 or bool(flags & FLAG_ISTFT)
        # 1. the framed kinds asked for, in the order their checks run; the last one is the plan's.  Any other mode asked for
        #    beside them travels as its bit, so that the library refuses the pair.
        kinds = [k for k, asked in (("imdct", imdct), ("adjoint", istft and stft_adjoint), ("istft", istft)) if asked][:1]
        kinds += ["istft_adjoint" if istft_adjoint else "spec" if stft_power is not None else "stft"] if stft and not kinds else []
        kinds += (["mdct"] if mdct and not imdct else []) + (["conv"] if conv is not None else [])
        foreign = ((FLAG_STFT if stft or mdct else 0) | (FLAG_DCT_ND if dctn else 0) | (FLAG_DCT if dct else 0) |
                   (FLAG_HALF_SPECTRUM if half_spectrum else 0))
        kind, framed_dims, words, lead = None, None, [], 0
        for kind in kinds:
            # 2. the kind's layout check, which gives the dims and the frame length of its request
            if kind == "imdct":
                framed_dims = _check_imdct_layout(in_shape, out_shape, imdct)
                req = FrameRequest(kind, 2 * imdct, imdct, window=stft_window, gain=imdct_gain)
            elif kind in ("istft", "adjoint"):
                if not int(istft_hop):
                    istft_hop = (flags & FLAG_STFT_HOP_MASK) >> 16
                    if stft_center is None:
                        stft_center = {0: None, FLAG_STFT_CENTER_ZEROS: "constant"}.get(
                            flags & (FLAG_STFT_CENTER_REFLECT | FLAG_STFT_CENTER_ZEROS), "reflect")
                check_layout = _check_stft_adjoint_layout if kind == "adjoint" else _check_istft_layout
                framed_dims = check_layout(in_shape, out_shape, istft_hop, stft_center)
                req = FrameRequest(kind, framed_dims[2], istft_hop, stft_center, stft_window, istft_gain, adjoint=stft_adjoint)
            elif kind == "istft_adjoint":  # (istft_adjoint = F beside stft_hop; the gain is istft_gain, the inverse plan's)
                if stft_power is not None or stft_fb is not None or stft_log is not None or stft_post is not None:
                    raise MifftError(ERR_UNSUPPORTED, "istft_adjoint with stft_power / stft_fb / stft_log / stft_post: the adjoint "
                                                      "of the inverse STFT stores complex bins")
                framed_dims = _check_istft_adjoint_layout(in_shape, out_shape, stft_hop, stft_center)
                if out_shape[1] != int(istft_adjoint):
                    raise MifftError(-2, f"istft_adjoint = {istft_adjoint} frames, out has {out_shape[1]}")
                req = FrameRequest(kind, framed_dims[1], stft_hop, stft_center, stft_window, istft_gain, frames=int(istft_adjoint))
            elif kind in ("stft", "spec"):
                if not int(stft_hop):
                    stft_hop = (flags & FLAG_STFT_HOP_MASK) >> 16
                    stft_center = {0: None, FLAG_STFT_CENTER_REFLECT: "reflect", FLAG_STFT_CENTER_ZEROS: "constant"}.get(
                        flags & (FLAG_STFT_CENTER_REFLECT | FLAG_STFT_CENTER_ZEROS), stft_center)
                if kind == "stft":
                    if stft_fb is not None:
                        raise MifftError(ERR_UNSUPPORTED, "stft_fb without stft_power: a filterbank applies to abs(X) ** power")
                    if stft_log is not None or stft_post is not None:
                        raise MifftError(ERR_UNSUPPORTED, "stft_log / stft_post without stft_power: they follow abs(X) ** power")
                    framed_dims = _check_stft_layout(in_shape, out_shape, stft_hop, stft_center)
                    req = FrameRequest(kind, framed_dims[1], stft_hop, stft_center, stft_window)
                else:
                    power = _spec_power(stft_power)
                    fbm = None if stft_fb is None else _fb_f64(stft_fb)
                    logv = None if stft_log is None else _spec_log(stft_log)
                    postm = None if stft_post is None else _post_f64(stft_post, None if fbm is None else int(fbm.shape[1]))
                    framed_dims = _check_spec_layout(in_shape, out_shape, stft_hop, stft_center, fbm, postm)
                    req = FrameRequest(kind, framed_dims[1], stft_hop, stft_center, stft_window, power=power, fb=fbm, log=logv,
                                       post=postm)
            elif kind == "mdct":
                framed_dims = _check_mdct_layout(in_shape, out_shape, mdct)
                req = FrameRequest(kind, 2 * mdct, mdct, window=stft_window, gain=mdct_scale)
            else:
                if len(in_shape) != 3 or len(out_shape) != 3 or in_shape[-1] != 1 or out_shape[-1] != 1:
                    raise MifftError(-1, f"convolution layouts are (batch, L, 1) -> (batch, Lo, 1), got {in_shape} -> {out_shape}")
                if in_shape[0] != out_shape[0] or out_shape[1] != conv.Lo:
                    raise MifftError(-2, f"x {in_shape} against out {out_shape} with Lo = {conv.Lo}")
                framed_dims, req = (in_shape[1], conv.n), conv
            if axes is not None:
                raise MifftError(ERR_UNSUPPORTED, _FRAMED_NO_AXES[kind])
            # 3. the payload; a forward tagged kind passes a power on as well, for the library to refuse
            bits, words, lead = _frame_payload(req)
            flags |= bits | foreign | (FLAG_STFT_POWER if kind in ("mdct", "conv") and stft_power is not None else 0)
            inverse = inverse or lead == 2
        stft, istft = lead == 1, lead == 2  # (which side of the family the plan is on)
        half_spectrum = bool(half_spectrum) or bool(int(flags) & FLAG_HALF_SPECTRUM)  # (the flag bit is the same request)
        dct = bool(dct) or bool(int(flags) & FLAG_DCT)
        dctn = bool(dctn) or bool(int(flags) & FLAG_DCT_ND)
        if dst and not (dct or dctn):
            raise MifftError(ERR_UNSUPPORTED, "dst=True selects the sine transform of a dct=True or dctn=True plan")
        if kinds:
            dims = framed_dims
        elif dctn:  # (with dct or half_spectrum as well: the library refuses the pair)
            dims = _check_dctn_layout(in_shape, out_shape)
            flags = (int(flags) | FLAG_DCT_ND | _dct_norm_flags(norm) | (FLAG_DCT if dct else 0) |
                     (FLAG_HALF_SPECTRUM if half_spectrum else 0))
            if dst:  # (the tag leads the first list; a type 4 travels as its own tag and the library refuses it)
                if bases is not None and len(bases) != len(dims):
                    raise MifftError(-7, "the bases list of an N-D DST plan has one entry per dim")
                tag = DST_TYPE4_TAG if dct_type == 4 else DST_TAG
                rest = [[int(b) for b in bs] for bs in bases] if bases is not None else [[] for _ in dims]
                bases = [[tag] + rest[0]] + rest[1:]
        elif dct:  # (with half_spectrum as well: the library refuses the pair)
            dims = _check_dct_layout(in_shape, out_shape)
            flags = int(flags) | FLAG_DCT | _dct_norm_flags(norm) | (FLAG_HALF_SPECTRUM if half_spectrum else 0)
            if dct_type == 4 or dst:  # (the tag, then the radices of n // 2; the tag alone: the default estimate)
                if bases is not None and len(bases) != 1:
                    raise MifftError(-7, "the bases list of a DCT plan has one entry, the radices of n // 2")
                tag = (DST_TYPE4_TAG if dct_type == 4 else DST_TAG) if dst else DCT_TYPE4_TAG
                bases = [[tag] + ([int(b) for b in bases[0]] if bases is not None else [])]
        elif half_spectrum:
            dims = _check_half_layout(in_shape, out_shape, bool(inverse))
            flags = int(flags) | FLAG_HALF_SPECTRUM
        else:
            _check_layout_conditions_nd(in_shape, out_shape)
            dims = out_shape[1:-1]
        if in_dtype not in _DTYPE_CODE or out_dtype not in _OUT_DTYPES:
            raise MifftError(-4, f"unsupported dtype {in_dtype} -> {out_dtype} (out_dtype must be floating point)")
        if bases is not None and len(bases) != len(dims):
            raise MifftError(-7, "The bases list should have the same outer size as the amount of internal "
                                 "dimensions. e.g. (batches, dim_0, dim_1, dim_2, 2) -> len(bases) == 3")
        flags = int(flags) | _keep_flags(len(out_shape), axes)
        self.in_dtype, self.out_dtype = in_dtype, out_dtype
        self.in_shape, self.out_shape = in_shape, out_shape
        self.inverse, self.device, self.flags = bool(inverse), int(device), int(flags)
        self.axes = None if axes is None else tuple(int(a) for a in axes)
        self.half_spectrum = bool(half_spectrum)
        self.dct = dct
        self.dctn = dctn
        self.stft = stft
        self.istft = istft
        self.spectrogram = kind == "spec"
        self.dct_type = int(dct_type) if dct and not dctn and not stft and not istft else 2
        self.dst = bool(dst) and (dct or dctn) and not stft and not istft
        self.mdct = mdct if kind == "mdct" else 0
        self.imdct = imdct if kind == "imdct" else 0
        self.stft_adjoint = int(stft_adjoint) if kind == "adjoint" else 0
        self.istft_adjoint = int(istft_adjoint) if kind == "istft_adjoint" else 0
        self.conv = conv
        self.conv_gates = getattr(conv, "gates", 0) if conv is not None else 0
        self._ndim = len(dims)
        c_dims = (ctypes.c_int64 * len(dims))(*dims)
        # 4. the payload and the radices as the lists of ``bases``, and the one call
        c_flat, c_len = _pack_bases(words, bases, lead)
        h = ctypes.c_void_p()
        # whole_batch > 0: this plan is one slab of a batch of that many transforms (mifft_plan_create_slab)
        self.whole_batch = int(whole_batch)
        check(_lib.lib().mifft_plan_create_slab(ctypes.byref(h), self.device, _DTYPE_CODE[in_dtype],
                                                _DTYPE_CODE[out_dtype], len(dims), c_dims, out_shape[0], in_shape[-1],
                                                int(self.inverse), c_flat, c_len, self.flags, self.whole_batch))
        self._h = h

    # -- introspection ------------------------------------------------------
    @property
    def ndim(self) -> int:
        return self._ndim

    def stages(self, dim: int) -> list:
        out = (ctypes.c_uint32 * 64)()
        k = check(_lib.lib().mifft_plan_stages(self._h, dim, out, 64))
        return list(out[:k])

    def kernel_name(self, dim: int) -> str:
        return _lib.lib().mifft_plan_kernel_name(self._h, dim).decode()

    @property
    def num_launches(self) -> int:
        return check(_lib.lib().mifft_plan_num_launches(self._h))

    def pass_geometry(self, dim: int, count: Optional[int] = None) -> tuple:
        """(tile, threads, n_tiles, grid) of the launch that an exec of ``count`` batch entries (default: the whole batch)
        makes for dimension ``dim``: transforms per workgroup tile, threads per workgroup, tiles, persistent workgroups.
        Workgroup w walks the tiles w, w + grid, ..; computed by the launch's own code (mifft_plan_pass_geometry).
        MifftError -15 for a kept dim or a pass that is not one persistent tile-kernel launch."""
        g = (ctypes.c_int64 * 4)()
        count = self.out_shape[0] if count is None else int(count)
        check(_lib.lib().mifft_plan_pass_geometry(self._h, int(dim), count, g))
        return tuple(int(v) for v in g)

    @property
    def in_bytes(self) -> int:
        return int(_lib.lib().mifft_plan_in_bytes(self._h))

    @property
    def out_bytes(self) -> int:
        return int(_lib.lib().mifft_plan_out_bytes(self._h))

    @property
    def scratch_bytes(self) -> int:
        """device bytes of the plan-owned scratch tensor (0 unless a long strided dimension or a three-launch
        four-step needs one; the reference's plan always owns one, fft/fft/_ndim_fft_gpu.mojo:185)"""
        return int(_lib.lib().mifft_plan_scratch_bytes(self._h))

    def device_status(self, ctx: Optional["DeviceContext"] = None) -> int:
        """Device-side error flags raised by execs of this plan (read and cleared; 0 = none).  Only the opt-in
        L2-resident image kernel can raise one (bounded XCD-barrier spin expired: bit 0; surplus workgroup: bit 1);
        synchronises the stream in that case only."""
        flags = ctypes.c_uint32(0)
        stream = (ctx.stream if ctx is not None else torch.cuda.current_stream(self.device)).cuda_stream
        check(_lib.lib().mifft_plan_device_status(self._h, stream, ctypes.byref(flags)))
        return int(flags.value)

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().mifft_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_fft(in_dtype, out_dtype, in_layout: Sequence[int], out_layout: Sequence[int], *, bases=None,
             inverse: bool = False, runtime_twfs: bool = True, max_cluster_size: int = 8,
             _test: Optional[GPUTest] = None, faithful_stages: bool = False,
             ctx: Optional[DeviceContext] = None, whole_batch: int = 0, half_spectrum: bool = False,
             axes: Optional[Sequence[int]] = None, dct: bool = False, norm=None, dctn: bool = False,
             dct_type: int = 2, dst: bool = False) -> Plan:
    """GPU overload of plan_fft (fft/fft/fft.mojo:161-210).

    ``runtime_twfs`` and ``max_cluster_size`` are accepted for call-site compatibility
    and ignored: twiddles always come from an fp64-accurate device table and CDNA4
    has no thread-block clusters.  ``bases=None`` selects the reference's GPU default.
    ``whole_batch`` (no reference counterpart): this plan covers one slab of a batch of that many transforms split over
    several plans / GPUs; size-dependent kernel choices follow the whole batch, so the slab's results equal the same
    rows of one plan over the whole batch bit for bit.
    ``half_spectrum`` (no reference counterpart): numpy's one-sided layouts, forward (batch, d0.., n, 1) ->
    (batch, d0.., n // 2 + 1, 2), inverse the other way round (include/mifft.h, MIFFT_FLAG_HALF_SPECTRUM).
    ``axes`` (no reference counterpart): the layout positions 1 .. rank - 2 to transform, None = all of them; the others
    are carried through untransformed (include/mifft.h, MIFFT_FLAG_KEEP_DIM).
    ``dct`` (no reference counterpart): DCT-II (``inverse``: its inverse) of the real rows of a (batch, n, 1) tensor into
    one of the same shape, ``norm`` None / "backward" / "ortho" as scipy.fft.dct (include/mifft.h, MIFFT_FLAG_DCT); ``bases``
    then factor n // 2, the packed transform the plan runs.  ``dct_type=4`` beside ``dct``: the DCT-IV (scipy's type 4; its
    own inverse up to the scale, in_dtype == out_dtype in both directions, MIFFT_DCT_TYPE4_TAG); the default is 2.
    ``dctn`` (no reference counterpart): the N-D DCT-II (``inverse``: its inverse) of a real (batch, d0.., 1) tensor into one of
    the same shape, over ``axes`` (None: every dim), ``norm`` as for ``dct`` (include/mifft.h, MIFFT_FLAG_DCT_ND).
    ``dst`` beside ``dct`` or ``dctn`` (no reference counterpart): the sine transform instead, DST-II / its inverse or with
    ``dct_type=4`` (``dct`` only) the DST-IV, as scipy.fft.dst / idst / dstn / idstn; layouts, ``bases``, ``norm`` and limits are
    those of the cosine plan (include/mifft.h, MIFFT_DST_TAG / MIFFT_DST_TYPE4_TAG).
    """
    del runtime_twfs, max_cluster_size
    if dst and not (dct or dctn):
        raise MifftError(ERR_UNSUPPORTED, "dst=True selects the sine transform of a dct=True or dctn=True plan")
    if dctn:  # (layout errors before any device work)
        _check_dctn_layout(tuple(int(v) for v in in_layout), tuple(int(v) for v in out_layout))
        _dct_norm_flags(norm)
    elif dct:
        _check_dct_layout(tuple(int(v) for v in in_layout), tuple(int(v) for v in out_layout))
        _dct_norm_flags(norm)
        if dct_type not in (2, 4):
            raise MifftError(ERR_UNSUPPORTED, f"dct_type must be 2 or 4, got {dct_type!r}")
    elif half_spectrum:
        _check_half_layout(tuple(int(v) for v in in_layout), tuple(int(v) for v in out_layout), bool(inverse))
    _keep_flags(len(out_layout), axes)
    if ctx is None:
        ctx = DeviceContext()
    flags = FLAG_FAITHFUL_STAGES if (faithful_stages or _test is not None) else 0
    return Plan(in_dtype, out_dtype, in_layout, out_layout, bases=bases, inverse=inverse,
                device=ctx.device, flags=flags, whole_batch=whole_batch, half_spectrum=half_spectrum, axes=axes,
                dct=dct, norm=norm, dctn=dctn, dct_type=dct_type if (dct and not dctn) or (dst and dctn) else 2,
                dst=dst)


def plan_stft(dtype, batch: int, length: int, n_fft: int, hop_length: int, *, window=None, center=None,
              ctx: Optional[DeviceContext] = None, whole_batch: int = 0) -> Plan:
    """Plan of the short-time Fourier transform of ``batch`` real signals of ``length`` samples (no reference counterpart;
    MIFFT_FLAG_STFT in include/mifft.h): frames of ``n_fft`` samples every ``hop_length``, multiplied by ``window`` (None:
    rectangular; else n_fft values as a sequence, numpy array or tensor, taken by value when the plan is made) and
    transformed to their n_fft // 2 + 1 non-negative bins.  ``center``: None (frame f starts at f * hop_length), "reflect" or
    "constant" (frame f is centred on f * hop_length; the signal is reflected, or continued by zeros, beyond both ends: torch's
    ``center=True`` with ``pad_mode``).  The plan has ``in_shape`` (batch, length, 1) and ``out_shape``
    (batch, F, n_fft // 2 + 1, 2), F = stft_frames(length, n_fft, hop_length, center), both of ``dtype`` (float32 / float64),
    and runs through ``fft(out, x, plan=plan)``, ``first=`` / ``count=`` included: one kernel launch, no padded copy, no tensor
    of frames.  Every argument error is raised before any device work."""
    batch, length, n_fft, hop_length = int(batch), int(length), int(n_fft), int(hop_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an STFT plan reads and writes float32 or float64, got {dtype}")
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with an odd n_fft or one below 8 ({n_fft}) is not supported")
    FLAG_STFT_HOP(hop_length)
    frames = stft_frames(length, n_fft, hop_length, _stft_center_flags(center) != 0)
    in_shape, out_shape = (batch, length, 1), (batch, frames, n_fft // 2 + 1, 2)
    _check_stft_layout(in_shape, out_shape, hop_length, center)
    if window is not None:
        window = _window_f64(window, n_fft)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, whole_batch=whole_batch, stft_hop=hop_length,
                stft_center=center, stft_window=window)


def plan_spectrogram(dtype, batch: int, length: int, n_fft: int, hop_length: int, *, window=None, center=None,
                     power=2.0, fb=None, ctx: Optional[DeviceContext] = None, whole_batch: int = 0, log=None,
                     amin: float = 1e-10, eps: float = 0.0, ref: float = 1.0, post=None) -> Plan:
    """Plan of the magnitude (``power=1``) or power (``power=2``) spectrogram of ``batch`` real signals of ``length`` samples
    (no reference counterpart; MIFFT_FLAG_STFT_POWER in include/mifft.h): plan_stft's frames, window and ``center``, but the
    one kernel stores abs(X) ** power as reals -- out_shape (batch, F, n_fft // 2 + 1, 1) -- or, with a filterbank ``fb`` of
    shape (n_fft // 2 + 1, M) (any real tensor or array, taken by value as float64; the orientation of
    torchaudio.functional.melscale_fbanks -- a librosa-style (M, n_fft // 2 + 1) matrix must be transposed by the caller), the
    M bands fb.T @ abs(X) ** power of every frame, out_shape (batch, F, M, 1).  The complex spectrogram is never written.  The
    filterbank is applied band by band over the span of each column's non-zero rows, so its cost follows the spans: a dense
    matrix is correct but slow.  ``melscale_fbanks`` makes a mel filterbank.
    ``log``: None, or a stage on every value v the plan would store, in the same launch -- "log": ln(max(v + eps, amin));
    "log10": the same in base 10 (Whisper's log10(max(mel, 1e-10)) is the default ``amin``); "db": torchaudio's
    amplitude_to_DB without top_db, mult * log10(max(v + eps, amin)) - mult * log10(max(amin, ref)) with mult 10 for
    ``power=2`` and 20 for ``power=1``.  ``ref`` with any other ``log`` is refused.  There is no ``top_db`` and no Whisper
    ``max - 8`` clamp: both need the maximum over a whole entry; apply them to the small output, e.g.
    ``y = torch.maximum(y, y.amax(dim=(-2, -1), keepdim=True) - 80.0)``.
    ``post``: an (M, Q) real matrix (needs ``fb``; taken by value as float64), applied to the M bands of every frame after the
    log stage, out_shape (batch, F, Q, 1): with ``create_dct`` the MFCC.  Needs M <= n_fft // 2 - 1.
    Runs through ``fft(out, x, plan=plan)``, ``first=`` / ``count=`` included; a frame's result is bit-identical for any batch
    and slab.  Every argument error is raised before any device work: ``power`` other than 1 or 2 is -15, a filterbank of
    another shape -2, an unknown ``log`` -15, a ``post`` of another row count than M -2, ``post`` without ``fb`` -15."""
    batch, length, n_fft, hop_length = int(batch), int(length), int(n_fft), int(hop_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"a spectrogram plan reads and writes float32 or float64, got {dtype}")
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with an odd n_fft or one below 8 ({n_fft}) is not supported")
    if power is None:
        raise MifftError(ERR_UNSUPPORTED, "power=None is the complex STFT: use plan_stft")
    power = _spec_power(power)
    FLAG_STFT_HOP(hop_length)
    frames = stft_frames(length, n_fft, hop_length, _stft_center_flags(center) != 0)
    if fb is not None:
        fb = _fb_f64(fb, n_fft // 2 + 1)
    logv = _log_stage(log, amin, eps, ref, power)
    if post is not None:
        post = _post_f64(post, None if fb is None else int(fb.shape[1]))
    in_shape = (batch, length, 1)
    width = n_fft // 2 + 1 if fb is None else int(fb.shape[1])
    out_shape = (batch, frames, width if post is None else int(post.shape[1]), 1)
    _check_spec_layout(in_shape, out_shape, hop_length, center, fb, post)
    if window is not None:
        window = _window_f64(window, n_fft)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, whole_batch=whole_batch, stft_hop=hop_length,
                stft_center=center, stft_window=window, stft_power=power, stft_fb=fb, stft_log=logv, stft_post=post)


def plan_istft(dtype, batch: int, frames: int, n_fft: int, hop_length: int, *, window=None, center=False,
               normalized: bool = False, length: Optional[int] = None, ctx: Optional[DeviceContext] = None,
               whole_batch: int = 0) -> Plan:
    """Plan of the inverse short-time Fourier transform with real output (no reference counterpart; MIFFT_FLAG_ISTFT in
    include/mifft.h; torch.istft's semantics): ``frames`` half spectra of ``n_fft // 2 + 1`` bins per batch entry are
    transformed back, multiplied by ``window`` (None: rectangular; else n_fft values, taken by value), overlap-added every
    ``hop_length`` samples and divided by the overlap-added squared window.  ``center``: the first and last n_fft // 2
    samples are trimmed (None / False, or True / "reflect" / "constant").  ``normalized``: the frames are multiplied by
    sqrt(n_fft).  ``length``: output samples per entry, default istft_length(frames, n_fft, hop_length, center); it may be
    shorter, never longer (no zero-padding).  The plan has ``in_shape`` (batch, frames, n_fft // 2 + 1, 2) and ``out_shape``
    (batch, length, 1), both of ``dtype`` (float32 / float64), and runs through ``fft(out, X, plan=plan)``, ``first=`` /
    ``count=`` included: one kernel launch, no tensor of frames, no memset; an entry's result is bit-identical for any batch
    and slab.  Every argument error is raised before any device work; a window that breaks the nonzero overlap-add condition
    in the output range is refused (-15)."""
    batch, frames, n_fft, hop_length = int(batch), int(frames), int(n_fft), int(hop_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an inverse STFT plan reads and writes float32 or float64, got {dtype}")
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with an odd n_fft or one below 8 ({n_fft}) is not supported")
    FLAG_STFT_HOP(hop_length)
    centred = _istft_center_flags(center) != 0
    T = istft_length(frames, n_fft, hop_length, centred) if length is None else int(length)
    in_shape, out_shape = (batch, frames, n_fft // 2 + 1, 2), (batch, T, 1)
    _check_istft_layout(in_shape, out_shape, hop_length, center)
    if window is not None:
        window = _window_f64(window, n_fft)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, whole_batch=whole_batch, istft_hop=hop_length,
                stft_center=center, stft_window=window, istft_gain=float(n_fft) ** 0.5 if normalized else 1.0)


def istft_schedule(plan: Plan, count: Optional[int] = None) -> list:
    """The walk of an inverse STFT plan's one launch over ``count`` batch entries (default: the whole batch), from
    ``pass_geometry(2, count)`` by host arithmetic alone: for every workgroup ``(first_tile, run_tiles, warmup_tiles)``.
    Tile t is tile t % tiles_per_entry of entry t // tiles_per_entry, tiles_per_entry = ceil(F / TILE) (the last tile of an
    entry is ragged); workgroup w owns the ascending run [first_tile, first_tile + run_tiles), lengths differing by one at
    most; a run that starts inside an entry at tile g first recomputes warmup_tiles = min(g, ceil((K - 1) / TILE)) tiles before
    it with the stores suppressed, K = ceil(n_fft / hop) the frames that cover one sample.
    An IMDCT plan (``plan_imdct``) walks the same runs over its tiles of ``pass_geometry(2)[0]`` frames; there the third value
    counts FRAMES, not tiles: a run that starts inside an entry transforms one frame, the last of the tile before it, with
    the stores suppressed (1), any other run none (0)."""
    if not getattr(plan, "istft", False):
        raise MifftError(ERR_UNSUPPORTED, "istft_schedule describes inverse STFT plans only")
    tile, _, n_tiles, grid = plan.pass_geometry(2, count)
    if getattr(plan, "imdct", 0):
        return _imdct_schedule(tile, n_tiles, grid, plan.in_shape[1])
    frames, n_fft = plan.in_shape[1], 2 * (plan.in_shape[2] - 1)
    hop = (plan.flags & FLAG_STFT_HOP_MASK) >> 16
    return _istft_schedule(tile, n_tiles, grid, frames, n_fft, hop)


def _istft_schedule(tile: int, n_tiles: int, grid: int, frames: int, n_fft: int, hop: int) -> list:
    tpe = -(-frames // tile)
    K = -(-n_fft // hop)
    W = -(-(K - 1) // tile)
    length, rem = divmod(n_tiles, grid)
    runs = []
    for w in range(grid):
        first = w * length + min(w, rem)
        runs.append((first, length + (1 if w < rem else 0), min(first % tpe, W)))
    return runs


def _imdct_schedule(tile: int, n_tiles: int, grid: int, frames: int) -> list:
    tpe = -(-frames // tile)
    length, rem = divmod(n_tiles, grid)
    runs = []
    for w in range(grid):
        first = w * length + min(w, rem)
        runs.append((first, length + (1 if w < rem else 0), 1 if first % tpe else 0))
    return runs


def _check_tensor(t: "torch.Tensor", shape: tuple, dtype, device: int, what: str) -> None:
    if not t.is_cuda or t.device.index != device:
        raise MifftError(-10, f"{what} must live on HIP device {device}, got {t.device}")
    if t.dtype != dtype or tuple(t.shape) != shape:
        raise MifftError(-14, f"{what} is {tuple(t.shape)} {t.dtype}, plan expects {shape} {dtype}")
    if not t.is_contiguous():
        raise MifftError(-14, f"{what} must be row-major contiguous")


def fft(output: "torch.Tensor", x: "torch.Tensor", ctx: Optional[DeviceContext] = None, *, plan: Plan,
        first: int = 0, count: Optional[int] = None) -> None:
    """GPU overload of fft (fft/fft/fft.mojo:262-323): enqueue on ctx's stream and return.

    Out of place; ``x`` is never written; every element of ``output`` (of the selected
    batch range) is written.  ``first``/``count`` select a slab of the leading dimension
    (used by the batch-sharded multi-GPU host); default is the whole batch.
    """
    if getattr(plan, "conv_gates", 0):
        raise MifftError(ERR_UNSUPPORTED, "a gated convolution plan takes its gates with every exec: "
                                          "plan.run(out, x, pregate=, postgate=) instead of fft(out, x, plan=plan)")
    if getattr(plan, "stft_adjoint", 0):
        raise MifftError(ERR_UNSUPPORTED, "an STFT adjoint plan takes its factor and edge tensors with every exec: "
                                          "plan.run(out, g, multiplier=, edge=) or plan.apply(g) instead of fft(out, x, plan=plan)")
    if ctx is None:
        ctx = DeviceContext(plan.device)
    io = getattr(plan, "io_dtype", None)  # (a half-storage convolution plan: 16-bit rows around float32 arithmetic)
    _check_tensor(x, plan.in_shape, io or plan.in_dtype, plan.device, "x")
    _check_tensor(output, plan.out_shape, io or plan.out_dtype, plan.device, "output")
    if count is None:
        count = plan.out_shape[0] - first
    check(_lib.lib().mifft_exec_batch(plan._h, x.data_ptr(), output.data_ptr(), int(first), int(count),
                                      ctx.stream.cuda_stream))


class StftAdjointPlan(Plan):
    """The adjoint of an STFT plan (``plan_stft_adjoint``; MIFFT_STFT_ADJ_TAG in include/mifft.h): the gradient with respect to
    the signal of ``stft`` (``multiplier`` None) or of the power / magnitude spectrogram (``multiplier`` 2 / 1), one launch.
    ``in_shape`` (batch, frames, n_fft // 2 + 1, 2), ``out_shape`` (batch, length, 1); ``mult_shape`` (batch, frames,
    n_fft // 2 + 1) with a multiplier, else None; ``edge_shape`` (batch, 2, n_fft // 2) with reflect padding, else None.
    ``covered`` = min(length, n_fft + hop (frames - 1) - c), c = n_fft // 2 when centred: the samples of every entry that
    ``run`` writes; the gradient of the others is zero."""

    def __init__(self, dtype, batch, length, n_fft, hop_length, window, center, multiplier, ctx):
        mode = {None: 1, 2: 2, 1: 3}[multiplier]
        centred = _stft_center_flags(center) != 0
        frames = stft_frames(length, n_fft, hop_length, centred)
        bins = n_fft // 2 + 1
        super().__init__(dtype, dtype, (batch, frames, bins, 2), (batch, length, 1), device=ctx.device, istft_hop=hop_length,
                         stft_center=center, stft_window=window, stft_adjoint=mode)
        self._ctx = ctx
        self.frames, self.multiplier, self.n_fft, self.hop_length, self.center = frames, multiplier, n_fft, hop_length, center
        self.mult_shape = (batch, frames, bins) if multiplier is not None else None
        self.edge_shape = (batch, 2, n_fft // 2) if center == "reflect" else None
        self._c = n_fft // 2 if centred else 0
        self.covered = min(length, n_fft + hop_length * (frames - 1) - self._c)

    def run(self, out: "torch.Tensor", g: "torch.Tensor", *, multiplier: Optional["torch.Tensor"] = None,
            edge: Optional["torch.Tensor"] = None, first: Optional[int] = None, count: Optional[int] = None) -> None:
        """The raw exec on the plan's stream: ``g`` (in_shape) is the incoming gradient -- or, on a plan with a multiplier,
        X itself, with the real gradient of abs(X) ** power as ``multiplier`` (mult_shape).  Writes out[:, :covered] and, on a
        reflect plan, the two strips of padded samples into ``edge`` (edge_shape; side 1 only below the frames' end) for the
        caller to fold; nothing else.  A tensor the plan needs and does not get is MifftError -12, one it has no use for -15,
        an input overlapping an output -13."""
        _check_tensor(g, self.in_shape, self.in_dtype, self.device, "g")
        _check_tensor(out, self.out_shape, self.out_dtype, self.device, "out")
        if multiplier is not None:
            _check_tensor(multiplier, self.mult_shape or tuple(multiplier.shape), self.out_dtype, self.device, "multiplier")
        if edge is not None:
            _check_tensor(edge, self.edge_shape or tuple(edge.shape), self.out_dtype, self.device, "edge")
        first = 0 if first is None else int(first)
        count = self.out_shape[0] - first if count is None else int(count)
        args = StftAdjArgs(STFT_ADJ_ARGS_MAGIC, g.data_ptr(), None if multiplier is None else multiplier.data_ptr(),
                           None if edge is None else edge.data_ptr())
        check(_lib.lib().mifft_exec_batch(self._h, ctypes.byref(args), out.data_ptr(), first, count,
                                          self._ctx.stream.cuda_stream))

    def apply(self, g: "torch.Tensor", multiplier: Optional["torch.Tensor"] = None) -> "torch.Tensor":
        """The whole gradient, (batch, length): allocates ``out`` and ``edge``, zero-fills the samples no frame covers, launches,
        and on a reflect plan adds the two flipped edge strips in place -- two torch ops on n_fft // 2 samples per row."""
        batch, T = self.out_shape[0], self.out_shape[1]
        with torch.cuda.stream(self._ctx.stream):
            out = torch.empty(self.out_shape, dtype=self.out_dtype, device=g.device)
            edge = None if self.edge_shape is None else torch.empty(self.edge_shape, dtype=self.out_dtype, device=g.device)
            if self.covered < T:
                out[:, self.covered:].zero_()
            self.run(out, g, multiplier=multiplier, edge=edge)
            gx = out.reshape(batch, T)
            if edge is not None:  # gx[t] += gxp[c - t], 1 <= t <= c;  gx[T - 2 - e] += gxp[c + T + e] for the e below the frames' end
                c = self._c
                gx[:, 1:c + 1] += edge[:, 0].flip(-1)
                e = min(c, self.n_fft + self.hop_length * (self.frames - 1) - c - T)
                if e > 0:
                    gx[:, T - 1 - e:T - 1] += edge[:, 1, :e].flip(-1)
        return gx


def plan_stft_adjoint(dtype, batch: int, length: int, n_fft: int, hop_length: int, *, window=None, center=None,
                      multiplier=None, ctx: Optional[DeviceContext] = None) -> StftAdjointPlan:
    """Plan of the adjoint of ``plan_stft(dtype, batch, length, n_fft, hop_length, window=, center=)`` (no reference counterpart;
    MIFFT_STFT_ADJ_TAG in include/mifft.h): the gradient of that plan's result with respect to its signal, an overlap-add of
    inverse real transforms without the envelope division, in ONE launch, no scratch, no memset, no atomics.  ``window`` and
    ``center`` (None, "reflect", "constant") are the forward plan's.  ``multiplier``: None -- ``run`` / ``apply`` take the
    incoming gradient g = dL/dRe X + i dL/dIm X, frames-major (batch, frames, n_fft // 2 + 1, 2); 2 or 1 (the power) -- they
    take X itself and the real gradient of abs(X) ** power, (batch, frames, n_fft // 2 + 1), which is multiplied in as the bins
    are loaded (2 m X, or m X / abs(X) with zero where abs(X) is).  An entry's result is bit-identical for any batch and slab.
    ``hop_length > n_fft`` and float64 frames beyond 10240 samples are refused (-15); every argument error is raised before any
    device work.  ``fft(out, x, plan=plan)`` refuses such a plan: use ``run`` or ``apply``."""
    batch, length, n_fft, hop_length = int(batch), int(length), int(n_fft), int(hop_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an STFT adjoint plan reads and writes float32 or float64, got {dtype}")
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with an odd n_fft or one below 8 ({n_fft}) is not supported")
    if multiplier is not None and (isinstance(multiplier, bool) or multiplier not in (1, 2)):
        raise MifftError(ERR_UNSUPPORTED, f"multiplier must be None, 2 (power) or 1 (magnitude), got {multiplier!r}")
    multiplier = None if multiplier is None else int(multiplier)
    FLAG_STFT_HOP(hop_length)
    _stft_center_flags(center)
    if window is not None:
        window = _window_f64(window, n_fft)
    if ctx is None:
        ctx = DeviceContext()
    return StftAdjointPlan(dtype, batch, length, n_fft, hop_length, window, center, multiplier, ctx)


def plan_istft_adjoint(dtype, batch: int, frames: int, n_fft: int, hop_length: int, *, window=None, center=False,
                       gain: float = 1.0, length: Optional[int] = None, ctx: Optional[DeviceContext] = None) -> Plan:
    """Plan of the adjoint of ``plan_istft(dtype, batch, frames, n_fft, hop_length, window=, center=, length=)`` (no reference
    counterpart; MIFFT_ISTFT_ADJ_TAG in include/mifft.h): the gradient of that plan's result with respect to its frames, the
    one-sided STFT of gy / envelope, in ONE launch, no scratch, no memset, no atomics.  ``window`` (None: rectangular) and
    ``center`` (None / False, or True / "constant") are the inverse plan's, ``gain`` its factor on the synthesis window
    (sqrt(n_fft) for ``normalized=True``), ``length`` its output samples per entry, default istft_length(frames, n_fft,
    hop_length, center).  The plan has ``in_shape`` (batch, length, 1), the incoming gradient gy, and ``out_shape``
    (batch, frames, n_fft // 2 + 1, 2), dL/dRe X + i dL/dIm X frames-major, both of ``dtype`` (float32 / float64), and runs
    through ``fft(out, gy, plan=plan)``, ``first=`` / ``count=`` included.  The load divides by the very envelope table the
    inverse plan divides by and selects zeros beyond both ends of [0, length): a frame that sees no stored sample is an exact
    zero, and so are the imaginary parts of bins 0 and n_fft // 2, which the inverse ignores.  A frame's result is
    bit-identical for any batch and slab.  Everything the inverse plan refuses is refused here -- ``hop_length > n_fft``, a
    ``length`` beyond what the frames cover, a window that breaks the nonzero overlap-add condition in the output range (-15)
    -- and so is ``center="reflect"``; every argument error is raised before any device work."""
    batch, frames, n_fft, hop_length = int(batch), int(frames), int(n_fft), int(hop_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an inverse STFT adjoint plan reads and writes float32 or float64, got {dtype}")
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"STFT with an odd n_fft or one below 8 ({n_fft}) is not supported")
    FLAG_STFT_HOP(hop_length)
    gain = float(gain)
    if not math.isfinite(gain) or gain == 0.0:
        raise MifftError(-5, f"the gain is finite and not zero, got {gain!r}")
    if center == "reflect":
        raise MifftError(ERR_UNSUPPORTED, "plan_istft_adjoint: center is None / False, True or \"constant\", not \"reflect\"")
    centred = _istft_center_flags(center) != 0
    T = istft_length(frames, n_fft, hop_length, centred) if length is None else int(length)
    in_shape, out_shape = (batch, T, 1), (batch, frames, n_fft // 2 + 1, 2)
    _check_istft_adjoint_layout(in_shape, out_shape, hop_length, center)
    if window is not None:
        window = _window_f64(window, n_fft)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, stft_hop=hop_length, stft_center=center,
                stft_window=window, istft_gain=gain, istft_adjoint=frames)


def time_fft(output: "torch.Tensor", x: "torch.Tensor", *, plan: Plan, iters: int = 10,
             ctx: Optional[DeviceContext] = None) -> float:
    """Average milliseconds per exec over ``iters`` back-to-back execs, measured with HIP
    events recorded on the launch stream inside the library (mifft_time_exec)."""
    if ctx is None:
        ctx = DeviceContext(plan.device)
    _check_tensor(x, plan.in_shape, plan.in_dtype, plan.device, "x")
    _check_tensor(output, plan.out_shape, plan.out_dtype, plan.device, "output")
    ms = ctypes.c_float()
    check(_lib.lib().mifft_time_exec(plan._h, x.data_ptr(), output.data_ptr(), ctx.stream.cuda_stream,
                                     int(iters), ctypes.byref(ms)))
    return float(ms.value)


# ---------------------------------------------------------------------------
# convenience wrappers: fftn / ifftn / rfftn(shape, radices) call surface
# ---------------------------------------------------------------------------

def _signal_device(x: "torch.Tensor", name: str) -> int:
    """the device of a wrapper's input, which has to be the HIP device its plan will be made on"""
    device = DeviceContext(x.device.index if x.is_cuda else None).device
    if not x.is_cuda or x.device.index != device:
        raise MifftError(-10, f"{name} must live on HIP device {device}, got {x.device}")
    return device


def _as_interleaved(x: "torch.Tensor"):
    """complex (batch, d0..) -> real view (batch, d0.., 2); real-typed input must already be (batch, d0.., C)."""
    if x.is_complex():
        return torch.view_as_real(x.contiguous()), True
    return x.contiguous(), False


_PLAN_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_PLAN_CACHE_SIZE = 32
_PLAN_CACHE_SCRATCH_BYTES = 8 << 30  # ... and at most this much plan-owned scratch (long-strided / three-launch routes)
_PLAN_CACHE_LOCK = threading.RLock()


def _table_digest(table) -> Optional[bytes]:
    """what a cache key holds of a contiguous float64 host table that its plan took by value (None: no table): the SHA-1 of
    its bytes, read in place"""
    return None if table is None else hashlib.sha1(table.numpy()).digest()


def _plan_cached(key_head: tuple, device: int, build, *tables, key_tail: tuple = ()) -> Plan:
    """The plan kept under ``key_head`` + the digests of the by-value ``tables`` + (device, the current stream's handle) +
    ``key_tail``, made by ``build()`` and inserted when there is none.  Called under _PLAN_CACHE_LOCK, which the caller holds
    until its launch is enqueued: the cache closes what it evicts.

    Plans of the convenience wrappers are kept (LRU): a plan is a few small device tables, building one
    costs a hipMalloc + copy per dimension, and its tables must outlive the kernels enqueued with it.

    A plan may own mutable device state that its execs share (the scratch tensor of the long-strided and three-launch
    four-step routes, the counters of the opt-in image kernel), so the C ABI allows ONE exec in flight per plan
    (include/mifft.h).  Execs are ordered on a stream; the cache therefore keeps one plan PER STREAM -- two streams (or
    two threads on their own streams) transforming the same shape never share a plan -- and is guarded by a lock."""
    for table in tables:  # (every cached call comes through here: a plain loop, _table_digest written out)
        key_head += (None if table is None else hashlib.sha1(table.numpy()).digest(),)
    key = key_head + (device, int(torch.cuda.current_stream(device).cuda_stream)) + key_tail
    plan = _PLAN_CACHE.get(key)
    if plan is None:
        plan = build()
        _plan_cache_insert(key, plan)
    else:
        _PLAN_CACHE.move_to_end(key)
    return plan


def _cached_plan(in_dtype, out_dtype, in_shape, out_shape, radices, inverse, faithful_stages, device,
                 half_spectrum: bool = False, axes=None, dct_flags: int = 0, dct_type: int = 2, dst: bool = False) -> Plan:
    """the cached plan_fft plan of the fftn / rfftn / dct families (takes the cache's lock, which is re-entrant: a caller that
    launches holds it already)"""
    # dct_flags: FLAG_DCT or FLAG_DCT_ND (| FLAG_DCT_ORTHO) of the dct / idct / dctn / idctn wrappers' plans, 0 for every other;
    # dct_type: 4 for the DCT-IV plans of dct / idct (the key of every other plan is what it has always been); dst: the sine
    # twins of dst / idst / dstn / idstn, whose keys alone grow by a word
    def build():
        common = dict(inverse=inverse, faithful_stages=faithful_stages, ctx=DeviceContext(device), half_spectrum=half_spectrum,
                      axes=axes)
        try:
            return plan_fft(in_dtype, out_dtype, in_shape, out_shape, bases=radices, dct=bool(dct_flags & FLAG_DCT),
                            dctn=bool(dct_flags & FLAG_DCT_ND), norm="ortho" if dct_flags & FLAG_DCT_ORTHO else None,
                            dct_type=dct_type, dst=dst, **common)
        except MifftError as e:
            # plan_fft keeps the reference's behaviour: its default radix estimate (trial division by 2..32 on the GPU,
            # primes <= 97 otherwise, fft/fft/fft.mojo:49-104) rejects lengths with a larger prime factor.  The
            # numpy-style wrappers are this repository's own surface, so they retry with the full prime factorisation.
            # (not for a DCT plan: a half length with a prime factor above 32 has been refused before the radix planning)
            if radices is not None or dct_flags or e.status not in (-5, -7):
                raise
            dims = _check_half_layout(in_shape, out_shape, inverse) if half_spectrum else in_shape[1:-1]
            bases = [_prime_factors(int(n)) if axes is None or p + 1 in axes else [] for p, n in enumerate(dims)]
            return plan_fft(in_dtype, out_dtype, in_shape, out_shape, bases=bases, **common)

    head = (in_dtype, out_dtype, in_shape, out_shape, None if radices is None else tuple(tuple(int(b) for b in r) for r in radices),
            bool(inverse), bool(faithful_stages))
    tail = ((bool(half_spectrum), _keep_flags(len(out_shape), axes), int(dct_flags)) + ((int(dct_type),) if dct_type != 2 else ()) +
            (("dst",) if dst else ()))
    with _PLAN_CACHE_LOCK:
        return _plan_cached(head, device, build, key_tail=tail)


def _plan_cache_insert(key, plan: Plan) -> None:
    """a new plan into the cache (under its lock), the oldest ones out while it is over its limits"""
    _PLAN_CACHE[key] = plan
    while len(_PLAN_CACHE) > 1 and (len(_PLAN_CACHE) > _PLAN_CACHE_SIZE or
                                    sum(q.scratch_bytes for q in _PLAN_CACHE.values()) > _PLAN_CACHE_SCRATCH_BYTES):
        _, old = _PLAN_CACHE.popitem(last=False)
        torch.cuda.synchronize(old.device)  # nothing enqueued with the evicted plan may still run
        old.close()


def _prime_factors(n: int) -> list:
    """distinct prime factors of n, ascending (a complete `bases` list for any length)"""
    f, d = [], 2
    while d * d <= n:
        if n % d == 0:
            f.append(d)
            while n % d == 0:
                n //= d
        d += 1
    if n > 1:
        f.append(n)
    return f


def clear_plan_cache() -> None:
    with _PLAN_CACHE_LOCK:
        for plan in _PLAN_CACHE.values():
            torch.cuda.synchronize(plan.device)
            plan.close()
        _PLAN_CACHE.clear()


def reduce_dims(shape: Sequence[int], dim) -> Optional[tuple]:
    """torch ``dim=`` on a logical shape -> the plan that computes it without moving data: ``(layout_dims, axes)`` with
    layout_dims = (batch, e0, .., ek) a reshape of ``shape`` and axes the layout positions (1 .. k + 1) to transform.
    None when nothing is transformed (an empty ``dim``, or only size-1 dims: the identity).  Rules, in order:
      1. size-1 dims are dropped (a length-1 transform is the identity);
      2. the dims before the first transformed one fold into the batch (a batch of 1 when dim 0 is transformed);
      3. runs of adjacent kept dims merge into one;
    and at most MAX_DIMS dims may remain between batch and C (MifftError -1 otherwise).  Negative dims count from the end;
    an out-of-range or repeated dim is MifftError -2.  Pure host logic: no tensor is touched."""
    shape = tuple(int(v) for v in shape)
    rank = len(shape)
    dims = (dim,) if isinstance(dim, int) else tuple(dim)
    norm = []
    for d in dims:
        d = int(d)
        if not -rank <= d < rank:
            raise MifftError(-2, f"dim {d} is out of range for a tensor of rank {rank}")
        norm.append(d % rank)
    if len(set(norm)) != len(norm):
        raise MifftError(-2, f"repeated dim in {tuple(dims)}")
    want = set(norm)
    kept_run = []  # (size, transformed) of the dims that remain, size-1 dims dropped
    for i, n in enumerate(shape):
        if n != 1:
            kept_run.append((n, i in want))
    first = next((k for k, (_, t) in enumerate(kept_run) if t), None)
    if first is None:
        return None
    batch = 1
    for n, _ in kept_run[:first]:
        batch *= n
    out, axes = [], []
    for n, t in kept_run[first:]:
        if t:
            out.append(n)
            axes.append(len(out))
        elif out and (len(out) not in axes):  # the previous dim is kept too: one merged dim
            out[-1] *= n
        else:
            out.append(n)
    if len(out) > MAX_DIMS:
        raise MifftError(-1, f"dim={tuple(dims)} on {shape} leaves {len(out)} dims after merging the kept ones; at most "
                             f"{MAX_DIMS} are supported")
    return (batch,) + tuple(out), tuple(axes)


def _dim_plan(logical: tuple, dim):
    """(layout dims, axes) of a wrapper call; dim=None: every dim but the first, as without ``dim`` (axes None)"""
    if dim is None:
        return logical, None
    r = reduce_dims(logical, dim)
    if r is None:
        return None, None
    dims, axes = r
    return dims, (None if len(axes) == len(dims) - 1 else axes)


def _run(x: "torch.Tensor", *, radices, inverse: bool, out_dtype, faithful_stages: bool, dim=None) -> "torch.Tensor":
    xr, was_complex = _as_interleaved(x)
    if out_dtype is None:
        out_dtype = xr.dtype if xr.dtype in (torch.float32, torch.float64) else torch.float64
    logical = tuple(xr.shape[:-1])
    comps = int(xr.shape[-1])
    layout, axes = _dim_plan(logical, dim)
    if layout is None:  # nothing to transform: a converted copy, as torch returns
        out = torch.zeros(logical + (2,), dtype=out_dtype, device=xr.device)
        out[..., :comps] = xr.to(out_dtype)
        return torch.view_as_complex(out) if was_complex else out
    xr = xr.reshape(layout + (comps,))
    out_shape = layout + (2,)
    out = torch.empty(out_shape, dtype=out_dtype, device=xr.device)
    # lookup AND enqueue under the cache lock: another thread that inserts a plan may evict (synchronise + close) only
    # plans that have nothing left to enqueue
    with _PLAN_CACHE_LOCK:
        plan = _cached_plan(xr.dtype, out_dtype, tuple(xr.shape), out_shape, radices, inverse, faithful_stages,
                                   xr.device.index, axes=axes)
        fft(out, xr, DeviceContext(xr.device.index), plan=plan)  # asynchronous on the current stream, like torch ops
    out = out.reshape(logical + (2,))
    return torch.view_as_complex(out) if was_complex else out


def fftn(x: "torch.Tensor", radices=None, *, out_dtype=None, faithful_stages: bool = False, dim=None) -> "torch.Tensor":
    """Forward C2C transform over every dim but the first (batch).  ``x``: complex
    ``(batch, d0..)`` or real-typed interleaved ``(batch, d0.., 2)``; ``radices``: one list per dim.
    ``dim``: torch's ``dim=`` on the logical shape (without the trailing 2 of interleaved input); dim 0 and negative dims
    allowed; the other dims are carried through untransformed (reduce_dims).  None: every dim but the first.  With
    ``dim``, ``radices`` has one list per dim of the reduced layout (an empty one for a kept dim).
    Asynchronous on the current torch stream; plans are cached per (shape, dtype, radices, dims, device, stream), so
    concurrent streams never share a plan's scratch (one exec in flight per plan, include/mifft.h)."""
    return _run(x, radices=radices, inverse=False, out_dtype=out_dtype, faithful_stages=faithful_stages, dim=dim)


def ifftn(x: "torch.Tensor", radices=None, *, out_dtype=None, faithful_stages: bool = False, dim=None) -> "torch.Tensor":
    """Inverse C2C transform (1/N per transformed dimension), same layout and ``dim`` rules as fftn."""
    return _run(x, radices=radices, inverse=True, out_dtype=out_dtype, faithful_stages=faithful_stages, dim=dim)


def _halved_dim(logical: tuple, dim) -> int:
    """the dim a one-sided transform halves: the last entry of ``dim`` (torch), which must be the innermost dim of size
    above 1 -- the library halves the last dimension of its layout"""
    rank = len(logical)
    last = (int(dim) if isinstance(dim, int) else int(tuple(dim)[-1])) % rank
    inner = max(i for i, n in enumerate(logical) if n != 1 or i == last)
    if last != inner:
        raise MifftError(ERR_UNSUPPORTED, f"a one-sided transform halves the last dim of `dim` ({last}); only the innermost "
                                          f"dim of size above 1 ({inner}) is supported")
    return last


def rfftn(x: "torch.Tensor", radices=None, *, out_dtype=None, faithful_stages: bool = False,
          onesided: bool = False, dim=None) -> "torch.Tensor":
    """Real-input transform: ``x`` is real ``(batch, d0..)``; returns the FULL spectrum as
    interleaved ``(batch, d0.., 2)`` like the reference (fft/fft/_fft.mojo:254-257), not numpy's half spectrum.
    ``onesided=True``: numpy's / torch's rfftn instead, complex ``(batch, d0.., n // 2 + 1)`` (an even last dim).
    ``dim``: as fftn; one-sided, the last entry of ``dim`` is the halved dim and must be the innermost one."""
    if x.is_complex():
        raise MifftError(-3, "rfftn expects a real tensor")
    if not onesided:
        return _run(x.unsqueeze(-1), radices=radices, inverse=False, out_dtype=out_dtype,
                    faithful_stages=faithful_stages, dim=dim)
    xr = x.unsqueeze(-1).contiguous()
    logical = tuple(x.shape)
    if out_dtype is None:
        out_dtype = xr.dtype if xr.dtype in (torch.float32, torch.float64) else torch.float64
    if dim is not None and len((dim,) if isinstance(dim, int) else tuple(dim)) > 0:
        _halved_dim(logical, dim)
    layout, axes = _dim_plan(logical, dim)
    if layout is None:
        return xr.squeeze(-1).to(out_dtype).to(torch.complex64 if out_dtype == torch.float32 else torch.complex128)
    xr = xr.reshape(layout + (1,))
    in_shape = tuple(xr.shape)
    out_shape = in_shape[:-2] + (in_shape[-2] // 2 + 1, 2)
    _check_half_layout(in_shape, out_shape, False)
    out = torch.empty(out_shape, dtype=out_dtype, device=xr.device)
    with _PLAN_CACHE_LOCK:
        plan = _cached_plan(xr.dtype, out_dtype, in_shape, out_shape, radices, False, faithful_stages,
                                   xr.device.index, half_spectrum=True, axes=axes)
        fft(out, xr, DeviceContext(xr.device.index), plan=plan)
    return torch.view_as_complex(out.reshape(logical[:-1] + (logical[-1] // 2 + 1, 2)))


def irfftn(X: "torch.Tensor", n: Optional[int] = None, radices=None, *, out_dtype=None, dim=None) -> "torch.Tensor":
    """Inverse of the one-sided rfftn (numpy.fft.irfftn(X, s=dims) over every dim but the first): ``X`` is complex
    ``(batch, d0.., h)`` or interleaved ``(batch, d0.., h, 2)``; ``n`` is the length of the last real dimension (default
    2 (h - 1); even, with n // 2 + 1 == h).  Returns real ``(batch, d0.., n)``, 1/N per dimension.  As numpy does, the
    imaginary parts of bins 0 and n / 2 of the last dimension are ignored (after the other dimensions are transformed).
    ``dim``: as fftn, on the complex logical shape; ``n`` applies to the last entry of ``dim``, which must be the
    innermost dim."""
    Xr = torch.view_as_real(X) if X.is_complex() else X
    if Xr.dim() < 3 or Xr.shape[-1] != 2:
        raise MifftError(-3, f"irfftn expects complex (batch, d0.., h) or interleaved (batch, d0.., h, 2), got "
                             f"{tuple(X.shape)} {X.dtype}")
    h = int(Xr.shape[-2])
    n = 2 * (h - 1) if n is None else int(n)
    if n % 2:
        raise MifftError(ERR_UNSUPPORTED, f"irfftn of an odd length ({n}) is not supported")
    if n // 2 + 1 != h:
        raise MifftError(-2, f"irfftn: n = {n} needs n // 2 + 1 = {n // 2 + 1} bins, X has {h}")
    if out_dtype is None:
        out_dtype = Xr.dtype if Xr.dtype in (torch.float32, torch.float64) else torch.float64
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"irfftn: out_dtype must be float32 or float64, got {out_dtype}")
    Xr = Xr.to(out_dtype).contiguous()  # (the inverse reads the plan's own float type)
    logical = tuple(Xr.shape[:-1])
    axes = None
    if dim is not None:
        if len((dim,) if isinstance(dim, int) else tuple(dim)) == 0:
            raise MifftError(-2, "irfftn: an empty dim has no last dim to take n from")
        _halved_dim(logical, dim)
        layout, axes = _dim_plan(logical, dim)
        Xr = Xr.reshape(layout + (2,))
    in_shape = tuple(Xr.shape)
    out_shape = in_shape[:-2] + (n, 1)
    _check_half_layout(in_shape, out_shape, True)
    out = torch.empty(out_shape, dtype=out_dtype, device=Xr.device)
    with _PLAN_CACHE_LOCK:
        plan = _cached_plan(out_dtype, out_dtype, in_shape, out_shape, radices, True, False, Xr.device.index,
                                   half_spectrum=True, axes=axes)
        fft(out, Xr, DeviceContext(Xr.device.index), plan=plan)
    return out.reshape(logical[:-1] + (n,))


def _dct_rows(x: "torch.Tensor", type: int, norm, out_dtype, dim: int, inverse: bool, kind: str = "dct") -> "torch.Tensor":
    """dct / idct and, with ``kind="dst"``, dst / idst: validation on the host, then one plan over the (batch, n, 1) view of ``x``"""
    name = ("i" if inverse else "") + kind
    if type not in (2, 4):
        raise MifftError(ERR_UNSUPPORTED, f"{name}: only types 2 and 4 are supported, got type={type!r}")
    dct_flags = FLAG_DCT | _dct_norm_flags(norm)
    if x.is_complex():
        raise MifftError(-3, f"{name} expects a real tensor")
    if x.dim() < 1:
        raise MifftError(-1, f"{name} expects a tensor of rank 1 or more")
    logical = tuple(x.shape)
    rank = len(logical)
    if not -rank <= int(dim) < rank:
        raise MifftError(-2, f"dim {dim} is out of range for a tensor of rank {rank}")
    last = int(dim) % rank
    inner = max(i for i, m in enumerate(logical) if m != 1 or i == last)
    if last != inner:
        raise MifftError(ERR_UNSUPPORTED, f"{name} along dim {last}: only the innermost dim of size above 1 ({inner}) is "
                                          f"supported")
    n = logical[last]
    batch = 1
    for i, m in enumerate(logical):
        batch *= m if i != last else 1
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"{name}: out_dtype must be float32 or float64, got {out_dtype}")
    if not inverse and x.dtype not in _DTYPE_CODE:
        raise MifftError(-4, f"{name}: unsupported input dtype {x.dtype}")
    shape = (batch, n, 1)
    _check_dct_layout(shape, shape)
    if inverse or type == 4:
        x = x.to(out_dtype)  # (the inverse, and the DCT-IV in both directions, read the plan's own float type)
    xr = x.contiguous().reshape(shape)
    device = DeviceContext(xr.device.index if xr.is_cuda else None).device
    out = torch.empty(shape, dtype=out_dtype, device=xr.device)
    with _PLAN_CACHE_LOCK:
        plan = _cached_plan(xr.dtype, out_dtype, shape, shape, None, inverse, False, device, dct_flags=dct_flags,
                                   dct_type=int(type), dst=kind == "dst")
        fft(out, xr, DeviceContext(device), plan=plan)
    return out.reshape(logical)


def dct(x: "torch.Tensor", type: int = 2, norm=None, *, out_dtype=None, dim: int = -1) -> "torch.Tensor":
    """scipy.fft.dct(x, type=2, norm=norm) along the last dim of a real tensor of any rank >= 1 (an even length from 8 on):
    ``X[k] = 2 sum_j x[j] cos(pi k (2j+1) / 2n)``; ``norm="ortho"`` scales X[0] by sqrt(1/4n) and the other bins by sqrt(1/2n).
    The leading dims fold into the batch; the result has the shape of ``x`` and dtype ``out_dtype`` (default: that of a float32 /
    float64 ``x``, else float64).  One kernel launch: n reals read once, n reals written once (MIFFT_FLAG_DCT).
    ``type=4`` is scipy's DCT-IV, ``X[k] = 2 sum_j x[j] cos(pi (2j+1)(2k+1) / 4n)``, ``norm="ortho"`` times sqrt(1/2n) (then
    its own inverse): one n // 2-point complex transform between two twiddles, the same limits, one launch; its input is
    converted to ``out_dtype`` first (MIFFT_DCT_TYPE4_TAG).  Only ``type=2`` and ``type=4``, and ``dim`` must be the innermost
    dim of size above 1 (MifftError -15 otherwise)."""
    return _dct_rows(x, type, norm, out_dtype, dim, False)


def idct(x: "torch.Tensor", type: int = 2, norm=None, *, out_dtype=None, dim: int = -1) -> "torch.Tensor":
    """scipy.fft.idct(x, type=2, norm=norm), the inverse of dct under the same ``norm``:
    ``x[j] = (X[0] + 2 sum_{k>=1} X[k] cos(pi k (2j+1) / 2n)) / 2n``.  Same layout, ``dim`` and dtype rules as dct; the input
    is converted to ``out_dtype`` first.  ``type=4``: dct(x, 4) / 2n (``norm="ortho"``: the orthonormal DCT-IV itself), the same
    kernel as the forward with another scale."""
    return _dct_rows(x, type, norm, out_dtype, dim, True)


def _dct_nd(x: "torch.Tensor", type: int, norm, dim, out_dtype, inverse: bool, kind: str = "dct") -> "torch.Tensor":
    """dctn / idctn and, with ``kind="dst"``, dstn / idstn: validation on the host, then one plan over the reduced
    (batch, e0.., 1) view of ``x``"""
    name = ("i" if inverse else "") + kind + "n"
    if type != 2:
        raise MifftError(ERR_UNSUPPORTED, f"{name}: only type 2 is supported, got type={type!r}")
    dct_flags = FLAG_DCT_ND | _dct_norm_flags(norm)
    if x.is_complex():
        raise MifftError(-3, f"{name} expects a real tensor")
    if x.dim() < 2:
        raise MifftError(-1, f"{name} expects a tensor of rank 2 or more: (batch, d0..)")
    logical = tuple(x.shape)
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"{name}: out_dtype must be float32 or float64, got {out_dtype}")
    if not inverse and x.dtype not in _DTYPE_CODE:
        raise MifftError(-4, f"{name}: unsupported input dtype {x.dtype}")
    r = reduce_dims(logical, tuple(range(1, len(logical))) if dim is None else dim)
    if r is None:  # nothing to transform: a converted copy
        return x.to(out_dtype, copy=True)
    layout, axes = r
    # a narrow input dtype goes to the plan only when the last dim is transformed (its row pass widens it); a plan whose
    # first pass is a column pass, and every inverse, reads the plan's own float type
    if inverse or (len(layout) - 1) not in axes:
        x = x.to(out_dtype)
    shape = layout + (1,)
    _check_dctn_layout(shape, shape)
    xr = x.contiguous().reshape(shape)
    device = DeviceContext(xr.device.index if xr.is_cuda else None).device
    out = torch.empty(shape, dtype=out_dtype, device=xr.device)
    with _PLAN_CACHE_LOCK:
        plan = _cached_plan(xr.dtype, out_dtype, shape, shape, None, inverse, False, device,
                                   axes=None if len(axes) == len(layout) - 1 else axes, dct_flags=dct_flags,
                                   dst=kind == "dst")
        fft(out, xr, DeviceContext(device), plan=plan)
    return out.reshape(logical)


def dctn(x: "torch.Tensor", type: int = 2, norm=None, *, dim=None, out_dtype=None) -> "torch.Tensor":
    """scipy.fft.dctn(x, type=2, norm=norm) over the dims ``dim`` of a real tensor of rank >= 2: the DCT-II of ``dct`` along
    each of them.  ``dim=None``: every dim but the first, as fftn; otherwise torch's ``dim=`` on the shape of ``x`` (dim 0 and
    negative dims allowed), resolved through reduce_dims: the other dims are carried through in place.  One kernel launch per
    transformed dim and no transposition (MIFFT_FLAG_DCT_ND): the innermost transformed dim, when it is the last dim of size
    above 1, runs the row kernel of ``dct`` (an even length from 8 on); every other one is transformed in place as pairs of
    adjacent real columns, at an even stride of at least 4 elements.  A float32 result takes any column length from 2 to 4096
    with prime factors up to 32; a float64 result every such length up to 2056 and, from 2058 up, only those the library has a
    three-pass column configuration for (4092 is the longest; 2058, 2080, 2100, 2401, 4000, 4095, 4096 and 150 more are
    refused with MifftError -15 "no fused column configuration").
    The result has the shape of ``x`` and dtype ``out_dtype`` (default: that of a float32 / float64 ``x``, else float64); a
    non-contiguous ``x`` is copied first; an empty ``dim`` or one of size-1 dims only returns a converted copy.  Only
    ``type=2`` (MifftError -15 otherwise); ``norm`` as in ``dct``."""
    return _dct_nd(x, type, norm, dim, out_dtype, False)


def idctn(x: "torch.Tensor", type: int = 2, norm=None, *, dim=None, out_dtype=None) -> "torch.Tensor":
    """scipy.fft.idctn(x, type=2, norm=norm), the inverse of dctn under the same ``norm`` and ``dim``; the input is converted
    to ``out_dtype`` first."""
    return _dct_nd(x, type, norm, dim, out_dtype, True)


def dst(x: "torch.Tensor", type: int = 2, norm=None, *, out_dtype=None, dim: int = -1) -> "torch.Tensor":
    """scipy.fft.dst(x, type=2, norm=norm) along the last dim of a real tensor of any rank >= 1 (an even length from 8 on):
    ``Y[k] = 2 sum_j x[j] sin(pi (k+1)(2j+1) / 2n)``; ``norm="ortho"`` scales the last bin Y[n-1] by sqrt(1/4n) and the other
    bins by sqrt(1/2n).  ``type=4`` is scipy's DST-IV, ``Y[k] = 2 sum_j x[j] sin(pi (2j+1)(2k+1) / 4n)``, ``norm="ortho"`` times
    sqrt(1/2n) (then its own inverse).  Each is the kernel of ``dct`` of that type with a sign in its load and the index
    reversal in its store: one launch, n reals read once and written once, the layout, ``dim``, dtype rules and limits of
    ``dct`` (MIFFT_DST_TAG, MIFFT_DST_TYPE4_TAG).  Only ``type=2`` and ``type=4`` (MifftError -15 otherwise)."""
    return _dct_rows(x, type, norm, out_dtype, dim, False, "dst")


def idst(x: "torch.Tensor", type: int = 2, norm=None, *, out_dtype=None, dim: int = -1) -> "torch.Tensor":
    """scipy.fft.idst(x, type=2, norm=norm), the inverse of dst under the same ``norm`` (the DST-III divided by 2n); the rules
    of idct.  ``type=4``: dst(x, 4) / 2n (``norm="ortho"``: the orthonormal DST-IV itself)."""
    return _dct_rows(x, type, norm, out_dtype, dim, True, "dst")


def dstn(x: "torch.Tensor", type: int = 2, norm=None, *, dim=None, out_dtype=None) -> "torch.Tensor":
    """scipy.fft.dstn(x, type=2, norm=norm) over the dims ``dim`` of a real tensor of rank >= 2: the DST-II of ``dst`` along
    each of them, on the passes of ``dctn`` -- one launch per transformed dim, the same ``dim``, lengths, strides and dtype
    rules (MIFFT_DST_TAG on a MIFFT_FLAG_DCT_ND plan).  Only ``type=2`` (MifftError -15 otherwise); a sine transform along one
    dim with a cosine transform along another is two calls."""
    return _dct_nd(x, type, norm, dim, out_dtype, False, "dst")


def idstn(x: "torch.Tensor", type: int = 2, norm=None, *, dim=None, out_dtype=None) -> "torch.Tensor":
    """scipy.fft.idstn(x, type=2, norm=norm), the inverse of dstn under the same ``norm`` and ``dim``; the input is converted
    to ``out_dtype`` first."""
    return _dct_nd(x, type, norm, dim, out_dtype, True, "dst")


def mdct_frames(length: int, n: int) -> int:
    """Frames an MDCT of ``n`` coefficients per frame makes of ``length`` samples: ceil(length / n) + 1.  Frame f covers the
    samples [(f - 1) n, (f + 1) n) with zeros outside [0, length), so every sample lies in two frames.  Pure host arithmetic."""
    length, n = int(length), int(n)
    if n < 1 or length < 1:
        raise MifftError(-2, f"mdct_frames: length and n are positive, got {length} and {n}")
    return (length + n - 1) // n + 1


def mdct_window(n: int) -> "torch.Tensor":
    """The sine window of an MDCT of ``n`` coefficients, sin(pi (j + 1/2) / 2n) for j < 2n, float64 on the host: it satisfies
    w[j] ** 2 + w[j + n] ** 2 = 1 (perfect reconstruction through imdct)."""
    n = int(n)
    if n < 1:
        raise MifftError(-2, f"mdct_window: n is positive, got {n}")
    return torch.sin(math.pi * (torch.arange(2 * n, dtype=torch.float64) + 0.5) / (2 * n))


def _mdct_fold_tables(n: int):
    """The fold of a frame of 2n windowed samples y to the n values u whose DCT-IV is twice the MDCT: u = sa * y[ia] + sb * y[ib]
    (u[i] = -y[3h-1-i] - y[3h+i] and u[h+i] = y[i] - y[n-1-i] for i < h = n // 2).  Returns (ia, sa, ib, sb), int64 / float64."""
    h = n // 2
    i = torch.arange(h, dtype=torch.int64)
    ia = torch.cat([3 * h - 1 - i, i])
    ib = torch.cat([3 * h + i, n - 1 - i])
    one = torch.ones(h, dtype=torch.float64)
    return ia, torch.cat([-one, one]), ib, torch.cat([-one, -one])


def _mdct_unfold_tables(n: int):
    """The unfold of v = DCT-IV(X) / 2 (n values) to the 2n samples of a frame, y[j] = sign[j] * v[idx[j]]:
    y[i] = v[h+i], y[n-1-i] = -v[h+i], y[3h-1-i] = -v[i], y[3h+i] = -v[i] for i < h = n // 2.  Returns (idx, sign)."""
    h = n // 2
    i = torch.arange(h, dtype=torch.int64)
    idx = torch.empty(2 * n, dtype=torch.int64)
    sign = torch.empty(2 * n, dtype=torch.float64)
    idx[i], sign[i] = h + i, 1.0
    idx[n - 1 - i], sign[n - 1 - i] = h + i, -1.0
    idx[3 * h - 1 - i], sign[3 * h - 1 - i] = i, -1.0
    idx[3 * h + i], sign[3 * h + i] = i, -1.0
    return idx, sign


def _mdct_n(n, who: str) -> int:
    n = int(n)
    if n % 2 or n < 8:
        raise MifftError(ERR_UNSUPPORTED, f"{who} with an odd n or one below 8 ({n}) is not supported")
    FLAG_STFT_HOP(n)
    return n


def _mdct_norm_scale(norm, n: int, who: str) -> float:
    """the factor on the plain cosine sum: 1, or sqrt(2 / n) for ``norm="ortho"`` (the orthonormal DCT-IV of the folded frame)"""
    if norm is None or norm == "backward":
        return 1.0
    if norm == "ortho":
        return math.sqrt(2.0 / n)
    raise MifftError(ERR_UNSUPPORTED, f"{who}: norm must be None, \"backward\" or \"ortho\", got {norm!r}")


def _check_mdct_layout(in_shape: tuple, out_shape: tuple, n: int) -> tuple:
    """Layouts of an MDCT plan (MIFFT_MDCT_TAG): x (batch, T, 1) real -> out (batch, F, n, 1) real with F = mdct_frames(T, n);
    returns the dims (T, 2n)."""
    if len(in_shape) != 3 or len(out_shape) != 4:
        raise MifftError(-1, f"MDCT layouts are (batch, T, 1) -> (batch, F, n, 1), got {in_shape} -> {out_shape}")
    if in_shape[-1] != 1 or out_shape[-1] != 1:
        raise MifftError(-3, f"both sides of an MDCT plan have 1 component, got {in_shape[-1]} and {out_shape[-1]}")
    if in_shape[0] != out_shape[0]:
        raise MifftError(-2, f"batch {in_shape[0]} of x against {out_shape[0]} of out")
    n = _mdct_n(n, "MDCT")
    T = in_shape[1]
    if T < 2:
        raise MifftError(-2, f"signals of {T} samples: at least 2")
    if out_shape[2] != n or out_shape[1] != mdct_frames(T, n):
        raise MifftError(-2, f"{T} samples make {mdct_frames(T, n)} frames of {n} coefficients, out is {out_shape}")
    return (T, 2 * n)


def plan_mdct(dtype, batch: int, length: int, n: int, *, window=None, norm=None, ctx: Optional[DeviceContext] = None,
              whole_batch: int = 0) -> Plan:
    """Plan of the MDCT of ``batch`` real signals of ``length`` samples (no reference counterpart; MIFFT_MDCT_TAG in
    include/mifft.h): ``n`` coefficients per frame of 2n samples, frames every n samples, multiplied by ``window`` (None: the
    sine window mdct_window(n); else 2n values, taken by value when the plan is made).  ``in_shape`` (batch, length, 1),
    ``out_shape`` (batch, mdct_frames(length, n), n, 1), both of ``dtype`` (float32 / float64); runs through
    ``fft(out, x, plan=plan)``, ``first=`` / ``count=`` included: one kernel launch, no padded copy, no tensor of frames.
    ``norm`` None / "backward" (the plain cosine sum) or "ortho" (times sqrt(2 / n)).  Every argument error is raised before
    any device work."""
    batch, length = int(batch), int(length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an MDCT plan reads and writes float32 or float64, got {dtype}")
    n = _mdct_n(n, "MDCT")
    scale = _mdct_norm_scale(norm, n, "plan_mdct")
    in_shape, out_shape = (batch, length, 1), (batch, mdct_frames(max(length, 1), n), n, 1)
    _check_mdct_layout(in_shape, out_shape, n)
    if window is not None:
        window = _window_f64(window, 2 * n)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, whole_batch=whole_batch, mdct=n, mdct_scale=scale,
                stft_window=window)


def mdct(x: "torch.Tensor", n: int, *, window=None, norm=None, out_dtype=None) -> "torch.Tensor":
    """The MDCT of a real ``x`` of shape (T,) or (..., T) with ``n`` coefficients per frame (frames of 2n samples every n):
    ``X[f, k] = sum_{j<2n} w[j] x~[(f - 1) n + j] cos(pi / n (j + 1/2 + n/2)(k + 1/2))``, x~ being x with zeros outside
    [0, T).  Returns (..., F, n) contiguous, F = mdct_frames(T, n); the leading dims fold into the batch.  ``window=None`` is
    the sine window; a tensor or sequence of 2n values is taken by value.  ``norm="ortho"`` multiplies by sqrt(2 / n) (the
    orthonormal DCT-IV of the folded frame).  n is even, from 8 to 16384 (float64: 12288), n // 2 without a prime factor above
    32.  Input that is not of ``out_dtype`` (default: that of a float32 / float64 ``x``, else float64) is converted first.
    One kernel launch: the framing, the window and the fold of 2n samples to n happen in the load of a DCT-IV tile.  Plans are
    cached per (shape, dtype, n, norm, device, stream) and the window's contents; loops should use ``plan_mdct``.
    Differentiable with respect to ``x`` (first order): when grad mode is on and ``x.requires_grad``, the result carries a
    ``grad_fn`` whose backward is ONE launch of the fused inverse (``plan_imdct`` with this call's scale as its gain, the same
    window and ``length=T``): the two plans are transposes of each other, so there is no kernel of its own.  The adjoint plan
    is made in the forward, under the key ``imdct`` itself uses, so that a refusal is a MifftError there.  Otherwise the call
    is what it has always been: same plan, same bits, no ``grad_fn``.  The window is taken by value and gets no gradient;
    there is no double backward."""
    if x.is_complex():
        raise MifftError(-3, "mdct expects a real tensor")
    if x.dim() < 1:
        raise MifftError(-1, "mdct expects a tensor of rank 1 or more: (T,) or (..., T)")
    n = _mdct_n(n, "mdct")
    scale = _mdct_norm_scale(norm, n, "mdct")
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"mdct: out_dtype must be float32 or float64, got {out_dtype}")
    T = int(x.shape[-1])
    if T < 2:
        raise MifftError(-2, f"mdct: signals of {T} samples: at least 2")
    w = None if window is None else _window_f64(window, 2 * n)
    device = _signal_device(x, "x")
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:  # (w: a fresh host table, kept by value)
        return _MDCTFunction.apply(x, (out_dtype, n, scale, None if w is None else w.clone(), device))
    return _mdct_exec(x, out_dtype, n, scale, w, device)


def _mdct_exec(x, dt, n: int, scale: float, w, device: int) -> "torch.Tensor":
    """the one launch of an accepted mdct call -- and of the backward of imdct, whose adjoint it is: x (..., T) -> (..., F, n)"""
    lead, T = tuple(x.shape[:-1]), int(x.shape[-1])
    frames = mdct_frames(T, n)
    in_shape, out_shape = (math.prod(lead), T, 1), (math.prod(lead), frames, n, 1)
    xr = x.to(dt).contiguous().reshape(in_shape)
    out = torch.empty(out_shape, dtype=dt, device=xr.device)
    with _PLAN_CACHE_LOCK:
        fft(out, xr, DeviceContext(device), plan=_mdct_plan(dt, in_shape, n, scale, w, device))
    return out.reshape(lead + (frames, n))


def _mdct_plan(dt, in_shape: tuple, n: int, scale: float, w, device: int) -> Plan:
    """the cached MDCT plan of signals (batch, T, 1) (under the cache's lock, which a caller that launches holds already)"""
    out_shape = (in_shape[0], mdct_frames(in_shape[1], n), n, 1)
    with _PLAN_CACHE_LOCK:
        return _plan_cached(("mdct", dt, in_shape, n, scale), device, lambda: Plan(
            dt, dt, in_shape, out_shape, device=device, mdct=n, mdct_scale=scale, stft_window=w), w)


def _imdct_plan(dt, in_shape: tuple, n: int, length: int, gain: float, w, device: int) -> Plan:
    """the cached IMDCT plan of frames (batch, F, n, 1) and ``length`` samples, likewise"""
    with _PLAN_CACHE_LOCK:
        return _plan_cached(("imdct", dt, in_shape, length, gain), device, lambda: Plan(
            dt, dt, in_shape, (in_shape[0], length, 1), device=device, imdct=n, imdct_gain=gain, stft_window=w), w)


class _MDCTFunction(torch.autograd.Function):
    """mdct with the gradient with respect to x.  The fold and the unfold are transposes of each other and the DCT-IV is
    symmetric, so the adjoint of the MDCT plan with scale s and window w on T samples is the IMDCT plan with gain s, the same
    w and length T: one launch, no kernel of its own.  First order."""

    @staticmethod
    def forward(ctx, x, call):
        dt, n, scale, w, device = call
        y = _mdct_exec(x, dt, n, scale, w, device)
        try:
            _imdct_plan(dt, (math.prod(y.shape[:-2]), int(y.shape[-2]), n, 1), n, int(x.shape[-1]), scale, w, device)
        except MifftError as e:
            raise MifftError(e.status, f"mdct: no gradient with respect to x for these arguments ({e}); the forward alone "
                                       f"works on an x without requires_grad (or under torch.no_grad())") from None
        ctx.call, ctx.x_shape, ctx.x_dtype = call, tuple(x.shape), x.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        dt, n, scale, w, device = ctx.call
        T, batch, frames = ctx.x_shape[-1], math.prod(ctx.x_shape[:-1]), int(gy.shape[-2])
        g = gy.to(dt).contiguous().reshape(batch, frames, n, 1)
        out = torch.empty((batch, T, 1), dtype=dt, device=g.device)
        with _PLAN_CACHE_LOCK:
            fft(out, g, DeviceContext(device), plan=_imdct_plan(dt, tuple(g.shape), n, T, scale, w, device))
        return out.reshape(ctx.x_shape).to(ctx.x_dtype), None


class _IMDCTFunction(torch.autograd.Function):
    """imdct with the gradient with respect to X: the adjoint of the IMDCT plan with gain g and window w, F frames and length T
    is the MDCT plan with scale g on gy, which yields mdct_frames(T, n) <= F frames; the frames beyond those see no stored
    sample and have a zero gradient.  One launch.  First order."""

    @staticmethod
    def forward(ctx, X, call):
        dt, n, gain, w, length, device = call
        lead, F = tuple(X.shape[:-2]), int(X.shape[-2])
        in_shape = (math.prod(lead), F, n, 1)
        Xr = X.to(dt).contiguous().reshape(in_shape)
        out = torch.empty((in_shape[0], length, 1), dtype=dt, device=Xr.device)
        with _PLAN_CACHE_LOCK:
            try:
                plan = _imdct_plan(dt, in_shape, n, length, gain, w, device)
                _mdct_plan(dt, (in_shape[0], _IMDCTFunction._adjoint_samples(in_shape[0], F, n, length), 1), n, gain, w, device)
            except MifftError as e:
                raise MifftError(e.status, f"imdct: no gradient with respect to X for these arguments ({e}); the forward alone "
                                           f"works on an X without requires_grad (or under torch.no_grad())") from None
            fft(out, Xr, DeviceContext(device), plan=plan)
        ctx.call, ctx.x_shape, ctx.x_dtype = call, tuple(X.shape), X.dtype
        return out.reshape(lead + (length,))

    @staticmethod
    def _adjoint_samples(batch: int, F: int, n: int, length: int) -> int:
        """samples per entry of the MDCT plan the backward runs: ``length`` -- or, with several entries AND a cropped length,
        the (F - 1) n samples that make all F frames (gy is continued by zeros to them: see backward)"""
        return length if mdct_frames(length, n) == F or batch == 1 else (F - 1) * n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        dt, n, gain, w, length, device = ctx.call
        lead, F = ctx.x_shape[:-2], ctx.x_shape[-2]
        batch, Fm = math.prod(lead), mdct_frames(length, n)
        g = gy.to(dt).contiguous().reshape(batch, length, 1)
        gX = torch.empty((batch, F, n, 1), dtype=dt, device=g.device)
        if Fm == F or batch == 1:  # the plan's frames are the first Fm of every entry: written in place, only the rest zero-filled
            gX[:, Fm:].zero_()
            with _PLAN_CACHE_LOCK:
                fft(gX[:, :Fm], g, DeviceContext(device), plan=_mdct_plan(dt, tuple(g.shape), n, gain, w, device))
        else:
            # (several entries whose rows are longer than the plan's: the plan stores Fm contiguous frames per entry, so gy is
            # continued by zeros to the (F - 1) n samples that make F frames -- the frames beyond Fm come out as exact zeros)
            gp = torch.zeros((batch, (F - 1) * n, 1), dtype=dt, device=g.device)
            gp[:, :length] = g
            with _PLAN_CACHE_LOCK:
                fft(gX, gp, DeviceContext(device), plan=_mdct_plan(dt, tuple(gp.shape), n, gain, w, device))
        return gX.reshape(ctx.x_shape).to(ctx.x_dtype), None


# ---------------------------------------------------------------------------
# fused FFT convolution of real rows
# ---------------------------------------------------------------------------

_FFTCONV_MAX = 16384
_FFTCONV_MODES = ("causal", "full", "same", "valid")


def _fftconv_ok(n: int) -> bool:
    """an FFT length the packed rows accept: even, 8 .. 16384, n // 2 without a prime factor above 32"""
    if n % 2 or n < 8 or n > _FFTCONV_MAX:
        return False
    h = n // 2
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while h % p == 0:
            h //= p
    return h == 1


@functools.lru_cache(maxsize=None)
def _fftconv_accepted(n: int, dtype) -> bool:
    """the library's own answer, from the checks it makes before it looks for a device (device -1 is none): the packed rows
    of float64 refuse some sixty lengths below 12288 that those of float32 take (434 is the first).  Asked once per (n, dtype)."""
    code = _DTYPE_CODE[dtype]
    h = ctypes.c_void_p()
    flat = (ctypes.c_uint32 * 8)(CONV_TAG_LO, CONV_TAG_HI, 1, 0, 1, 0, 16, 0)
    rc = _lib.lib().mifft_plan_create(ctypes.byref(h), -1, code, code, 2, (ctypes.c_int64 * 2)(2, n), 1, 1, 0, flat,
                                      (ctypes.c_int32 * 2)(8, 0), FLAG_STFT)
    return rc == -10


def _fftconv_check_length(who: str, what: str, n: int, dtype) -> None:
    """the one refusal of an FFT length (``what``: the argument it came in), before any device work"""
    if not (_fftconv_ok(n) and _fftconv_accepted(n, dtype)):
        raise MifftError(ERR_UNSUPPORTED, f"{who}: {what} = {n} is no accepted FFT length (even, 8 .. 16384, float64 to 12288, "
                                          "n // 2 without a prime factor above 32): see fftconv_length")


class ConvRequest(NamedTuple):
    """What a convolution plan is asked for (``Plan(conv=)``): the FFT length ``n``, ``D`` filter rows, the stored samples
    ``o`` .. of ``Lo`` per row; on an overlap-save plan ``S`` > 0 samples stored per block from sample ``o`` (= c) of its
    result on, ``F`` blocks per row and the first block's start ``s0`` (a single block: 0, 1, 0); ``Q`` > 0 taps per partition
    and ``P`` partitions on a partitioned one; the ``mode`` word, the device ``address`` of the filter spectra, the ``gates`` bits.  ``grad``: the
    filter gradient of that convolution instead, in ``partials`` sums per channel (0: the library's choice), ``gates`` fused
    into its loads of x and gy.  ``stage`` (with ``grad``): 0 that fused gradient; 1 / 2 the spectra of its u-blocks / g-blocks
    stored instead of summed, 3 the lag-group correlation over such spectra (``o`` = the stored u-frames per row, ``S`` = the lag
    groups, ``F`` = ``Lo`` = the g-blocks per row, ``s0`` = the index of the first stored u-frame) -- the three plans of a
    ``FusedPartConvGradPlan`` (word 10 of the payload; include/mifft.h)."""
    n: int
    D: int
    o: int
    Lo: int
    S: int = 0
    F: int = 1
    s0: int = 0
    Q: int = 0
    P: int = 0
    mode: int = 0
    address: int = 0
    gates: int = 0
    grad: bool = False
    partials: int = 0
    stage: int = 0


def _conv_payload(r: ConvRequest) -> list:
    """The payload words of a request, MIFFT_CONV_TAG's 8 (a single block), 12 (overlap-save), 16 (either, gated) or 20
    (partitioned) or MIFFT_CONV_GRAD_TAG's 16 (include/mifft.h); status -5 for a value that does not fit its word.  Pure: no
    device, no library call."""
    r = ConvRequest(*(int(v) for v in r))
    blocks = r.S > 0 or r.Q > 0
    fields = ("D", "o", "Lo", "mode") + (("S", "F") if blocks else ())
    for what in fields:
        if not 0 <= getattr(r, what) < 1 << 32:
            raise MifftError(-5, f"{what} = {getattr(r, what)} of a convolution plan does not fit an unsigned 32-bit word")
    if blocks and not -(1 << 31) <= r.s0 < 1 << 31:
        raise MifftError(-5, f"s0 = {r.s0} of a convolution plan does not fit a signed 32-bit word")
    if r.gates not in (0, 1, 2, 3):
        raise MifftError(-5, f"conv_gates = {r.gates}: bit 0 the pregate, bit 1 the postgate (1, 2 or 3)")
    for what in ("Q", "P", "partials"):
        if not 0 <= getattr(r, what) < 1 << 32:
            raise MifftError(-5, f"{what} = {getattr(r, what)} of a convolution plan does not fit an unsigned 32-bit word")
    if r.stage not in (0, 1, 2, 3) or (r.stage and not r.grad):
        raise MifftError(-5, f"stage = {r.stage} of a convolution plan: 0, or 1 / 2 / 3 on a filter-gradient request")
    if r.grad:  # (always the block geometry: a single block stores its Lo samples)
        return [CONV_GRAD_TAG_LO, CONV_GRAD_TAG_HI, r.D, r.o, r.S or r.Lo, r.mode, r.F, r.s0 & 0xFFFFFFFF, r.Lo, r.partials,
                r.stage, r.gates, 0, 0, 0, 0]
    words = [CONV_TAG_LO, CONV_TAG_HI, r.D, r.o, r.S if blocks else r.Lo, r.mode, r.address & 0xFFFFFFFF, (r.address >> 32) & 0xFFFFFFFF]
    if blocks:
        words += [r.F, r.s0 & 0xFFFFFFFF, r.Lo, r.gates]
    elif r.gates:  # (word 8, F, is 0 for the single block: o and Lo are words 3 and 4)
        words += [0, 0, 0, r.gates]
    if r.gates or r.Q:
        words += [0, 0, 0, 0]
    if r.Q:
        words += [r.Q, r.P, 0, 0]
    return words


class ConvPairRequest(NamedTuple):
    """What a two-signal convolution plan is asked for (``Plan(conv=)``; MIFFT_CONV_PAIR_TAG in include/mifft.h): the FFT
    length ``n``, ``K`` samples per row of v, the indices ``ea`` / ``eb`` at which a row of x / of v starts inside its n
    zero-extended samples, the stored samples ``o`` .. of ``Lo`` per row, the ``mode`` word (bit 0: correlate)."""
    n: int
    K: int
    ea: int
    eb: int
    o: int
    Lo: int
    mode: int = 0


def _conv_pair_payload(r: ConvPairRequest) -> list:
    """The 16 payload words of a two-signal request; status -5 for a value that does not fit its word.  Pure."""
    r = ConvPairRequest(*(int(v) for v in r))
    for what in ("K", "ea", "eb", "o", "Lo", "mode"):
        if not 0 <= getattr(r, what) < 1 << 32:
            raise MifftError(-5, f"{what} = {getattr(r, what)} of a two-signal convolution plan does not fit an unsigned 32-bit word")
    return [CONV_PAIR_TAG_LO, CONV_PAIR_TAG_HI, r.K, r.ea, r.eb, r.o, r.Lo, r.mode] + [0] * 8


def _fftconv_pair_window(mode: str, L: int, K: int, correlate: bool) -> tuple:
    """(ea, eb, o, Lo) of a mode of ``fftconv_pair``: scipy.signal's crops of the full convolution / correlation of L and K
    samples ("causal": the first L samples of the plain product, lags 0 .. L - 1 of a correlation)"""
    if mode == "causal":
        return 0, 0, 0, L
    o, Lo = _fftconv_window(mode, L, K)
    return (K - 1 if correlate else 0), 0, o, Lo


def _fftconv_pair_adjoints(L: int, K: int, ea: int, eb: int, o: int, Lo: int, correlate: bool) -> tuple:
    """The two gradient plans of the pair plan (L, K, ea, eb, o, Lo, correlate), each as (first operand, La, Lb, ea', eb', o',
    Lo', correlate') with the first operand "gy" or "x" and the second the other saved tensor: gx = pair(gy, v), gv =
    pair(gy, x) -- or, of a correlation, pair(x, gy).  Exact adjoints, circular case included: the embedding offset of gy is the
    forward's o, so nothing is padded."""
    if not correlate:
        return ("gy", Lo, K, o, eb, ea, L, True), ("gy", Lo, L, o, ea, eb, K, True)
    return ("gy", Lo, K, o, eb, ea, L, False), ("x", L, Lo, ea, o, eb, K, True)


def fftconv_length(m: int, dtype=torch.float32) -> int:
    """The smallest FFT length n >= m that a fused convolution plan of ``dtype`` accepts (even, 8 .. 16384, n // 2 without a
    prime factor above 32; float64 plans stop at 12288 and skip a few lengths more).  MifftError beyond the last one: longer
    convolutions run as overlap-save blocks (fftconv_block, plan_fftconv(taps=))."""
    m = int(m)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"fftconv_length: float32 or float64, got {dtype}")
    n = max(m + (m & 1), 8)
    while n <= _FFTCONV_MAX:
        if _fftconv_ok(n) and _fftconv_accepted(n, dtype):
            return n
        n += 2
    raise MifftError(ERR_UNSUPPORTED, f"fftconv_length({m}): no accepted FFT length up to {_FFTCONV_MAX}; longer convolutions "
                                      "run as overlap-save blocks (fftconv_block, plan_fftconv(taps=), fftconv(block=))")


# the measured time per block sample of the overlap-save kernel at every block length, in hundredths of the cheapest
# (profiles/r17_fftconv_long.txt, the sweep at 33 taps)
_FFTCONV_BLOCK_COST = {
    torch.float32: {256: 100, 512: 136, 1024: 148, 2048: 154, 4096: 133, 8192: 179, 16384: 166},
    torch.float64: {256: 100, 512: 109, 1024: 117, 2048: 133, 4096: 163, 8192: 200},
}


def fftconv_block(K: int, dtype=torch.float32) -> int:
    """The FFT length of the overlap-save blocks ``fftconv`` picks for a filter of ``K`` taps: among the powers of two from 256
    to 16384 (float64: 8192) with n >= 2 (K - 1), the one with the least w(n) n / (n - K + 1) -- the block samples transformed
    per stored sample, times w(n), the measured time per block sample of the kernel of that length (_FFTCONV_BLOCK_COST;
    DESIGN.md 3.4n) --, the smaller on a tie.  MifftError when there is none (K > 8193, float64 4097): a filter longer than half a block needs
    partitioned convolution (``partition=``; fftconv_partition)."""
    K = int(K)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"fftconv_block: float32 or float64, got {dtype}")
    if K < 1:
        raise MifftError(-2, f"fftconv_block: a filter of K = {K} taps (at least 1)")
    best, best_cost = None, None
    for n, w in sorted(_FFTCONV_BLOCK_COST[dtype].items()):
        if n >= 2 * (K - 1):
            cost = Fraction(w * n, n - K + 1)  # (exact: a tie is a tie)
            if best is None or cost < best_cost:
                best, best_cost = n, cost
    if best is None:
        raise MifftError(ERR_UNSUPPORTED, f"fftconv_block({K}): no block of up to {8192 if dtype == torch.float64 else _FFTCONV_MAX} "
                                          "points holds two filter lengths; filters longer than half a block need partitioned "
                                          "convolution: fftconv(..., partition=\"auto\") or plan_fftconv(..., taps=K, partition=Q) "
                                          "(see fftconv_partition)")
    return best


def fftconv_partition(K: int, dtype=torch.float32) -> tuple:
    """(n, Q) of the partitioned convolution ``fftconv(partition="auto")`` picks for a filter of ``K`` taps that no
    overlap-save block holds: ``n`` the largest power-of-two block of ``dtype`` (16384; float64 8192) and ``Q = n // 2 + 1`` taps
    per partition, so that every block of n samples stores S = n - Q + 1 = n // 2 samples and the filter has
    P = ceil(K / Q) partitions -- the fewest transforms per stored sample among the pairs (n, Q).  The rule
    does not look at K; MifftError for K < 1, for more than 2^30 taps after rounding up to whole partitions, or for another
    dtype."""
    K = int(K)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"fftconv_partition: float32 or float64, got {dtype}")
    if K < 1:
        raise MifftError(-2, f"fftconv_partition: a filter of K = {K} taps (at least 1)")
    n = 8192 if dtype == torch.float64 else _FFTCONV_MAX
    Q = n // 2 + 1
    if -(-K // Q) * Q > 1 << 30:
        raise MifftError(ERR_UNSUPPORTED, f"fftconv_partition({K}): more than 2^30 taps in whole partitions of {Q}")
    return n, Q


class ConvPlan(Plan):
    """The plan of ``plan_fftconv``: a ``Plan`` that owns the tensor of filter spectra its kernel reads.
    ``filter_spectrum`` is (channels, n // 2 + 1, 2) of the plan's dtype, zero-filled at first; its address is bound into
    the plan and never changes, its contents may be rewritten between execs in stream order.
    An overlap-save plan (``plan_fftconv(taps=K)``) has ``taps`` = K, ``step`` = n - K + 1 samples stored per block and
    ``blocks`` per row; a single-block plan has ``taps`` and ``step`` None and one block.
    A gated plan (``plan_fftconv(pregate=True)`` and / or ``postgate=True``) has ``pregate`` / ``postgate`` True and runs
    through ``run``, which takes the gate tensors of that exec; ``fft(out, x, plan=plan)`` refuses it.
    A partitioned plan (``plan_fftconv(taps=K, partition=Q)``) has ``partition`` = Q taps per partition, ``partitions`` =
    ceil(K / Q), ``step`` = n - Q + 1 and a ``filter_spectrum`` of (channels, partitions, n // 2 + 1, 2): partition p holds
    rfft(k[p Q : (p + 1) Q], n).  ``partition`` is None and ``partitions`` 1 on every other plan.
    A half-storage plan (``plan_fftconv(torch.float32, ..., io_dtype=torch.bfloat16)`` or ``torch.float16``) has that
    ``io_dtype``: ``x``, the gates and ``out`` are tensors of it, widened in the kernel's load and rounded once, to nearest
    even, in its store; ``filter_spectrum`` and the arithmetic stay float32.  ``io_dtype`` is None on every other plan."""

    def __init__(self, dtype, batch, channels, length, n, offset, out_length, correlate, ctx, taps=None, pregate=False,
                 postgate=False, partition=None, io_dtype=None):
        self.ctx = ctx
        self.io_dtype = io_dtype
        self.channels, self.length, self.n = channels, length, n
        self.offset, self.out_length, self.correlate = offset, out_length, bool(correlate)
        self.taps, self.step, self.blocks = taps, None, 1
        self.partition, self.partitions = partition, 1
        self.pregate, self.postgate = bool(pregate), bool(postgate)
        if partition is not None:
            self.partitions = -(-taps // partition)
        with torch.cuda.stream(ctx.stream):
            shape = (channels, n // 2 + 1, 2) if partition is None else (channels, self.partitions, n // 2 + 1, 2)
            self.filter_spectrum = torch.zeros(shape, dtype=dtype, device=f"cuda:{ctx.device}")
        req = _fftconv_request(n, channels, offset, out_length, correlate, taps, partition, io_dtype)
        self.step, self.blocks = req.S or None, req.F
        super().__init__(dtype, dtype, (batch * channels, length, 1), (batch * channels, out_length, 1), device=ctx.device,
                         conv=req._replace(address=self.filter_spectrum.data_ptr(),
                                           gates=(1 if self.pregate else 0) | (2 if self.postgate else 0)))

    def run(self, out: "torch.Tensor", x: "torch.Tensor", *, pregate: Optional["torch.Tensor"] = None,
            postgate: Optional["torch.Tensor"] = None, first: Optional[int] = None, count: Optional[int] = None) -> None:
        """The exec of a gated plan, enqueued on the plan's stream: ``out[r] = postgate[r] * conv(pregate[r] * x[r])`` for the
        signal rows ``first`` .. ``first + count - 1`` (default: all).  ``pregate`` has ``in_shape``, ``postgate`` ``out_shape``,
        both of the plan's dtype (``io_dtype`` where the plan has one, as ``x`` and ``out`` then are), contiguous, on its device;
        each is given exactly where the plan has it.  All four tensors
        are the WHOLE batch's: the library offsets them by ``first`` rows.  A gate may alias ``x``, not ``out``; none is written."""
        if not self.conv_gates:
            raise MifftError(ERR_UNSUPPORTED, "run() is the exec of a gated plan (plan_fftconv(pregate=True) / postgate=True); "
                                              "this plan runs through fft(out, x, plan=plan)")
        for t, want, what in ((pregate, self.pregate, "pregate"), (postgate, self.postgate, "postgate")):
            if want and t is None:
                raise MifftError(-12, f"the plan has a {what}: run(..., {what}=) is missing")
            if not want and t is not None:
                raise MifftError(ERR_UNSUPPORTED, f"the plan has no {what}: plan_fftconv(..., {what}=True) makes one that has")
        sdt = self.io_dtype or self.in_dtype
        _check_tensor(x, self.in_shape, sdt, self.device, "x")
        _check_tensor(out, self.out_shape, sdt, self.device, "out")
        if pregate is not None:
            _check_tensor(pregate, self.in_shape, sdt, self.device, "pregate")
        if postgate is not None:
            _check_tensor(postgate, self.out_shape, sdt, self.device, "postgate")
        first = 0 if first is None else int(first)
        count = self.out_shape[0] - first if count is None else int(count)
        args = GatedArgs(GATED_ARGS_MAGIC, x.data_ptr(), pregate.data_ptr() if pregate is not None else None,
                         postgate.data_ptr() if postgate is not None else None)
        check(_lib.lib().mifft_exec_batch(self._h, ctypes.addressof(args), out.data_ptr(), first, count,
                                          self.ctx.stream.cuda_stream))

    def set_filter(self, k: "torch.Tensor") -> None:
        """``k`` real, (channels, K) or (K,) (one filter for every channel), K <= n: writes rfft(k, n) into
        ``filter_spectrum`` with the library's own one-sided rfftn, on the plan's stream."""
        if k.is_complex() or k.dim() not in (1, 2):
            raise MifftError(-3, f"set_filter expects a real (channels, K) or (K,) tensor, got {tuple(k.shape)} {k.dtype}")
        if k.dim() == 2 and k.shape[0] != self.channels:
            raise MifftError(-2, f"set_filter: {k.shape[0]} filters for {self.channels} channels")
        K = int(k.shape[-1])
        if self.partition is not None:  # (P spectra per channel: partition p is rfft(k[p Q : (p + 1) Q], n), the last zero-filled)
            P, Q = self.partitions, self.partition
            if K < 1 or K > self.taps:
                raise MifftError(-2, f"set_filter: a filter of K = {K} taps on a partitioned plan of taps = {self.taps} (1 <= K <= taps)")
            with torch.cuda.stream(self.ctx.stream):
                kq = torch.zeros((self.channels, P * Q), dtype=self.out_dtype, device=self.filter_spectrum.device)
                kq[:, :K] = k.to(device=kq.device, dtype=self.out_dtype)
                kp = torch.zeros((self.channels * P, self.n), dtype=self.out_dtype, device=kq.device)
                kp[:, :Q] = kq.reshape(self.channels * P, Q)
                H = rfftn(kp, onesided=True)
                self.filter_spectrum.copy_(torch.view_as_real(H).reshape(self.filter_spectrum.shape))
            return
        if K < 1 or K > self.n:
            raise MifftError(-2, f"set_filter: a filter of K = {K} taps does not fit the FFT length n = {self.n} (1 <= K <= n)")
        if self.taps is not None and K > self.taps:
            raise MifftError(-2, f"set_filter: a filter of K = {K} taps on an overlap-save plan of taps = {self.taps}: the blocks "
                                 "would wrap around")
        with torch.cuda.stream(self.ctx.stream):
            kp = torch.zeros((self.channels, self.n), dtype=self.out_dtype, device=self.filter_spectrum.device)
            kp[:, :K] = k.to(device=kp.device, dtype=self.out_dtype)
            H = rfftn(kp, onesided=True)
            self.filter_spectrum.copy_(torch.view_as_real(H))

    def add_skip(self, d) -> None:
        """adds the skip term ``d`` -- a float, or a real (channels,) tensor -- to every bin of ``filter_spectrum``, on the
        plan's stream: conv(x, h) + d x = conv(x, h') with h'[0] = h[0] + d, whose spectrum is H + d (d is real, so the same
        holds for the conjugate a correlation multiplies by).  Call it after ``set_filter``, which overwrites the spectrum.
        On a partitioned plan d goes to partition 0 alone, which holds tap 0."""
        with torch.cuda.stream(self.ctx.stream):
            if isinstance(d, torch.Tensor):
                if d.is_complex() or tuple(d.shape) != (self.channels,):
                    raise MifftError(-2, f"add_skip expects a float or a real ({self.channels},) tensor, got {tuple(d.shape)} {d.dtype}")
                d = d.to(device=self.filter_spectrum.device, dtype=self.out_dtype).reshape(self.channels, 1)
            if self.partition is not None:
                self.filter_spectrum[:, 0, :, 0] += d
            else:
                self.filter_spectrum[:, :, 0] += d

    def set_filter_spectrum(self, Hc: "torch.Tensor") -> None:
        """copies a spectrum the caller already holds -- complex (channels, n // 2 + 1) or interleaved (.., 2), the
        unnormalised rfft(k, n); on a partitioned plan (channels, partitions, n // 2 + 1), one spectrum per partition -- into
        ``filter_spectrum``, on the plan's stream"""
        Hr = torch.view_as_real(Hc) if Hc.is_complex() else Hc
        if tuple(Hr.shape) != tuple(self.filter_spectrum.shape):
            raise MifftError(-2, f"set_filter_spectrum expects {tuple(self.filter_spectrum.shape[:-1])} complex values, "
                                 f"got {tuple(Hc.shape)} {Hc.dtype}")
        with torch.cuda.stream(self.ctx.stream):
            self.filter_spectrum.copy_(Hr.to(device=self.filter_spectrum.device, dtype=self.out_dtype))


def _io_mode_bits(io_dtype) -> int:
    """bits 8..15 of a convolution payload's mode word: the code of the storage type, 0 without one"""
    return 0 if io_dtype is None else _DTYPE_CODE[io_dtype] << 8


def _check_io_dtype(who: str, dtype, io_dtype) -> None:
    """``io_dtype`` is None, or bfloat16 / float16 beside ``dtype`` = float32 (status -4 otherwise)"""
    if io_dtype is None:
        return
    if io_dtype not in _IO_DTYPES:
        raise MifftError(-4, f"{who}: io_dtype is torch.bfloat16 or torch.float16 (or None), got {io_dtype}")
    if dtype != torch.float32:
        raise MifftError(-4, f"{who}: io_dtype = {io_dtype} stores 16-bit rows around float32 arithmetic: dtype must be "
                             f"torch.float32, got {dtype}")


def _fftconv_ols_geometry(n: int, K: int, offset: int, out_length: int, correlate: bool) -> tuple:
    """(c, S, s0, F) of an overlap-save plan: S = n - K + 1 samples per block are free of wrap-around, from c = K - 1 on
    (correlation: from 0 on); block 0 starts c samples before the first wanted one"""
    S = n - K + 1
    c = 0 if correlate else K - 1
    return c, S, offset - c, -(-out_length // S)


def _fftconv_part_geometry(n: int, Q: int, K: int, offset: int, out_length: int, correlate: bool) -> tuple:
    """(c, S, s0, F, P) of a partitioned plan: P = ceil(K / Q) partitions of Q taps; the overlap-save geometry of a filter of Q
    taps -- S = n - Q + 1 samples per block free of wrap-around, from c = Q - 1 on (correlation: from 0 on)"""
    return _fftconv_ols_geometry(n, Q, offset, out_length, correlate) + (-(-K // Q),)


def _fftconv_request(n: int, channels: int, offset: int, out_length: int, correlate: bool, taps, partition, io_dtype) -> ConvRequest:
    """the request of ``plan_fftconv``'s / ``plan_fftconv_grad``'s arguments; address, gates and partials are the plan's to add"""
    r = ConvRequest(n, channels, offset, out_length, mode=(1 if correlate else 0) | _io_mode_bits(io_dtype))
    if taps is None:
        return r
    if partition is None:
        c, S, s0, F = _fftconv_ols_geometry(n, taps, offset, out_length, correlate)
        return r._replace(o=c, S=S, F=F, s0=s0)
    c, S, s0, F, P = _fftconv_part_geometry(n, partition, taps, offset, out_length, correlate)
    return r._replace(o=c, S=S, F=F, s0=s0, Q=partition, P=P)


def _fftconv_plan_args(who: str, kind: str, dtype, batch, channels, length, n, taps, offset, out_length, correlate, partition,
                       io_dtype) -> tuple:
    """The argument checks ``plan_fftconv`` and ``plan_fftconv_grad`` (``who``; ``kind`` its noun) share, all before any
    device work: (batch, channels, length, n, taps, offset, out_length, partition) as integers, ``out_length`` defaulted."""
    batch, channels, length, n, offset = int(batch), int(channels), int(length), int(n), int(offset)
    out_length = length if out_length is None else int(out_length)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"a {kind} plan reads and writes float32 or float64, got {dtype}")
    _check_io_dtype(who, dtype, io_dtype)
    if batch < 1 or channels < 1:
        raise MifftError(-8, f"{who}: batch = {batch} and channels = {channels} must be positive")
    _fftconv_check_length(who, "n", n, dtype)
    if partition is not None:  # (``taps`` = K in partitions of Q taps)
        if taps is None:
            raise MifftError(-2, f"{who}: partition = {partition} goes with taps = K, the length of the filter")
        taps, partition = int(taps), int(partition)
        if partition < 1 or partition > n - 1:
            raise MifftError(-2, f"{who}: partition = {partition} taps per partition at the block length n = {n}: 1 <= partition <= n - 1")
        if taps < 1 or -(-taps // partition) * partition > 1 << 30:
            raise MifftError(-2, f"{who}: taps = {taps} in partitions of {partition}: 1 <= taps, and at most 2^30 taps in whole partitions")
    elif taps is not None:
        taps = int(taps)
        if taps < 1 or taps > n - 1:
            raise MifftError(-2, f"{who}: taps = {taps} at the block length n = {n}: 1 <= taps <= n - 1")
    if taps is None:  # (a single block: everything inside the FFT length)
        if length < 2 or length > n:
            raise MifftError(ERR_UNSUPPORTED, f"{who}: rows of {length} samples at n = {n}: 2 <= length <= n")
        if offset < 0 or out_length < 1 or offset + out_length > n:
            raise MifftError(-5, f"{who}: offset = {offset}, out_length = {out_length}: 0 <= offset, 1 <= out_length, "
                                 f"offset + out_length <= n = {n}")
    else:  # (blocks: the window lies in the full linear result; a partitioned plan bounds out_length as well)
        if length < 2 or length > 1 << 30:
            raise MifftError(ERR_UNSUPPORTED, f"{who}: rows of {length} samples: 2 <= length <= 2^30")
        full = length if correlate else length + taps - 1
        cap = partition is not None and out_length > 1 << 30
        if offset < 0 or out_length < 1 or offset + out_length > full or cap:
            raise MifftError(-5, f"{who}: offset = {offset}, out_length = {out_length}: 0 <= offset, 1 <= out_length"
                                 f"{' <= 2^30' if partition is not None else ''}, "
                                 f"offset + out_length <= {full} (the {'correlation' if correlate else 'full convolution'} of "
                                 f"{length} samples with {taps} taps)")
    return batch, channels, length, n, taps, offset, out_length, partition


def plan_fftconv(dtype, batch: int, channels: int, length: int, n: int, *, taps: Optional[int] = None, offset: int = 0,
                 out_length: Optional[int] = None, correlate: bool = False, ctx: Optional[DeviceContext] = None,
                 pregate: bool = False, postgate: bool = False, partition: Optional[int] = None, io_dtype=None) -> ConvPlan:
    """Plan of the fused FFT convolution (no reference counterpart; MIFFT_CONV_TAG in include/mifft.h) of ``batch * channels``
    real rows of ``length`` samples, row-major (batch, channels, length), at the FFT length ``n`` (see fftconv_length):
    ``y[r] = irfft(rfft(x[r], n) * G[r % channels], n)[offset : offset + out_length]`` in ONE kernel launch, G the plan's
    ``filter_spectrum`` (``correlate``: its conjugate).  ``out_length`` defaults to ``length``.  ``in_shape``
    (batch * channels, length, 1), ``out_shape`` (batch * channels, out_length, 1), both of ``dtype`` (float32 / float64);
    runs through ``fft(out, x, plan=plan)``, ``first=`` / ``count=`` included.  ``n < length + K - 1`` gives the circular
    result.  Every argument error is raised before any device work.
    ``taps=K`` makes it an overlap-save plan at the block length ``n``, still one launch: filters of up to K taps,
    1 <= K <= n - 1, on rows of any ``length`` >= 2; every block of n samples stores its n - K + 1 samples that no wrap-around
    touched.  ``offset`` / ``out_length`` are then coordinates in the full linear convolution of length + K - 1 samples
    (``correlate``: in y[t] = sum_j k[j] x[t + j], t < length), wholly inside it.
    ``pregate`` / ``postgate`` = True make it a gated plan (the 16-word payload), of either kind:
    ``y[r] = b[r] * conv(a[r] * x[r])`` with a tensor ``a`` of ``in_shape`` and / or ``b`` of ``out_shape`` given with every
    exec, multiplied into the kernel's load and store -- still one launch, no intermediate.  Such a plan runs through
    ``plan.run(out, x, pregate=a, postgate=b)``.  A skip term d * (a * x) is d added to every bin of ``filter_spectrum``.
    ``partition=Q`` (with ``taps=K``) makes it a partitioned plan (the 20-word payload), for filters longer than half a block:
    ``taps`` may then be any K >= 1, 1 <= Q <= n - 1; the filter is cut into ceil(K / Q) partitions of Q taps, every block of n
    samples stores n - Q + 1, and the kernel transforms one shifted input block per live partition for every block it stores
    -- still one launch and no intermediate, but the work grows with K / Q.  Gates as above (``run``); without them ``fft``.
    ``io_dtype`` = torch.bfloat16 or torch.float16 (with ``dtype`` = torch.float32 only) makes it a half-storage plan of any
    of these kinds: ``x``, the gates and ``out`` are tensors of ``io_dtype``, widened exactly in the load and rounded once
    (to nearest even) in the store; the arithmetic and ``filter_spectrum`` stay float32, and the result equals the float32
    plan's on the widened tensors, rounded with ``.to(io_dtype)``, bit for bit.  Still one launch and no intermediate.
    The plan-level API carries no autograd; ``plan_fftconv_grad`` of the same arguments is the plan of its filter gradient,
    and the opposite-``correlate`` plan on rows of ``out_length`` samples its input gradient (what ``fftconv`` does)."""
    batch, channels, length, n, taps, offset, out_length, partition = _fftconv_plan_args(
        "plan_fftconv", "convolution", dtype, batch, channels, length, n, taps, offset, out_length, correlate, partition, io_dtype)
    return ConvPlan(dtype, batch, channels, length, n, offset, out_length, correlate, DeviceContext() if ctx is None else ctx, taps=taps,
                    pregate=pregate, postgate=postgate, partition=partition, io_dtype=io_dtype)


def _fftconv_pick(who: str, L: int, K: int, dtype, n: Optional[int], block: Optional[int]) -> tuple:
    """(n, taps) of ``fftconv``'s two paths for rows of L samples and K taps: the single block at the FFT length n (taps None),
    or overlap-save blocks of n points (taps = K) -- forced by ``block``, or chosen when L + K - 1 is beyond the last single
    length.  Every refusal of the pair (n, block) is raised here, for ``fftconv`` and for what mirrors its choice."""
    if block is not None and n is not None:
        raise ValueError(f"{who}: n is the FFT length of the single-block path, block that of the overlap-save path: not both")
    taps = None
    if block is not None:
        n, taps = int(block), K
    elif n is None:
        try:
            n = fftconv_length(L + K - 1, dtype)
        except MifftError as e:
            if e.status != ERR_UNSUPPORTED:
                raise
            n, taps = fftconv_block(K, dtype), K
    else:
        n = int(n)
    if taps is not None and K > n - 1:
        raise MifftError(-2, f"{who}: a filter of K = {K} taps does not fit overlap-save blocks of {n} points (K <= block - 1)")
    if K > n:
        raise MifftError(-2, f"{who}: a filter of K = {K} taps does not fit the FFT length n = {n}")
    _fftconv_check_length(who, "n", n, dtype)
    if taps is None and L > n:
        raise MifftError(ERR_UNSUPPORTED, f"{who}: rows of {L} samples are longer than the FFT length n = {n}")
    return n, taps


def _fftconv_pick_part(who: str, L: int, K: int, dtype, n: Optional[int], block: Optional[int], partition) -> tuple:
    """(n, taps, Q): ``_fftconv_pick`` when ``partition`` is None (Q None: today's paths and refusals); an integer Q forces
    the partitioned path at ``block`` (default: the largest power-of-two block of the dtype); "auto" takes the existing path
    whenever there is one and fftconv_partition(K) otherwise.  ``partition`` excludes ``n``."""
    if partition is None:
        return _fftconv_pick(who, L, K, dtype, n, block) + (None,)
    if n is not None:
        raise ValueError(f"{who}: n is the FFT length of the single-block path, partition belongs to the blocks of the "
                         "partitioned path (block=): not both")
    if isinstance(partition, str):
        if partition != "auto":
            raise ValueError(f"{who}: partition is None, a number of taps per partition or \"auto\", got {partition!r}")
        try:
            return _fftconv_pick(who, L, K, dtype, None, block) + (None,)
        except MifftError as e:
            if e.status != ERR_UNSUPPORTED or block is not None or K <= (4097 if dtype == torch.float64 else 8193):
                raise  # (a refusal of the arguments, not the want of a block that holds two filter lengths)
        n, Q = fftconv_partition(K, dtype)
    else:
        Q = int(partition)
        n = int(block) if block is not None else (8192 if dtype == torch.float64 else _FFTCONV_MAX)
    _fftconv_check_length(who, "block", n, dtype)
    if Q < 1 or Q > n - 1:
        raise MifftError(-2, f"{who}: partition = {Q} taps per partition does not fit blocks of {n} points (1 <= partition <= block - 1)")
    return n, K, Q


def _fftconv_window(mode: str, L: int, K: int) -> tuple:
    """(offset, out_length) of scipy.signal.fftconvolve's crops of the full convolution of L and K samples"""
    if mode == "causal":
        return 0, L
    if mode == "full":
        return 0, L + K - 1
    if mode == "same":
        return (K - 1) // 2, L
    return min(L, K) - 1, max(L, K) - min(L, K) + 1  # "valid"


def _fftconv_dtypes(x: "torch.Tensor", io_dtype) -> tuple:
    """(the working dtype, what x, the gates and the result are in memory): float32 around ``io_dtype``; else x's own float
    type, or float64"""
    dtype = torch.float32 if io_dtype is not None else x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    return dtype, io_dtype or dtype


def _fftconv_selector(n: int, taps, Q) -> dict:
    """the ``n`` / ``block`` / ``partition`` arguments that make ``fftconv`` take the path (n, taps, Q) again"""
    return {"block": n, "partition": Q} if Q is not None else {"block": n} if taps is not None else {"n": n}


def _fftconv_fwd_plan(dtype, rows, D, L, n, taps, offset, out_length, correlate, device, gates, Q=None, io_dtype=None):
    """the cached forward plan of ``fftconv`` (the caller holds _PLAN_CACHE_LOCK)"""
    return _plan_cached(("fftconv", dtype, rows, D, L, n, offset, out_length, bool(correlate)), device, lambda: plan_fftconv(
        dtype, rows // D, D, L, n, taps=taps, offset=offset, out_length=out_length, partition=Q, correlate=correlate,
        ctx=DeviceContext(device), pregate=bool(gates & 1), postgate=bool(gates & 2), io_dtype=io_dtype),
        key_tail=(taps, gates, Q, io_dtype))


def _fftconv_exec(plan: ConvPlan, out, x, k, skip, pregate=None, postgate=None) -> None:
    """one call's use of a cached plan: the filter's spectrum, the skip term, the launch (gated: ``run``)"""
    plan.set_filter(k)
    if skip is not None:
        plan.add_skip(skip)
    if plan.conv_gates:
        plan.run(out, x, pregate=pregate, postgate=postgate)
    else:
        fft(out, x, DeviceContext(plan.device), plan=plan)


def fftconv(x: "torch.Tensor", k: "torch.Tensor", *, n: Optional[int] = None, mode: str = "causal",
            correlate: bool = False, block: Optional[int] = None, pregate: Optional["torch.Tensor"] = None,
            postgate: Optional["torch.Tensor"] = None, skip=None, partition=None, io_dtype=None) -> "torch.Tensor":
    """Convolution by FFT along the last dim of a real ``x`` of shape (..., D, L) with ``k`` of shape (D, K), one filter per
    channel, or of shape (..., L) with a 1-D ``k``: one kernel launch per call (plus the transform of the filter).
    ``n`` is the FFT length, default fftconv_length(L + K - 1); a smaller one gives the circular result.
    ``mode="causal"`` returns the first L samples (the Hyena / S4 convention); "full", "same" and "valid" are
    scipy.signal.fftconvolve's crops.  ``correlate=True`` (with "causal" only) returns y[t] = sum_j k[j] x[t + j], the adjoint
    of the causal convolution.  float32 / float64; other input is converted to float64.
    Differentiable, first order: when grad mode is on and ``x``, ``k``, ``pregate``, ``postgate`` or a tensor ``skip`` requires
    grad, the call goes through a torch.autograd.Function whose forward is this same code (the same kernels, the same bits)
    and whose backward computes only the gradients asked for: the gradient of ``x`` and ``pregate`` by ONE launch of the
    opposite-``correlate`` plan on the incoming gradient (``postgate`` fused into its load; ``pregate`` into its store when
    only ``x`` wants a gradient), the gradient of ``k`` and ``skip`` by the fused filter-gradient kernel
    (``fftconv_filter_grad``; the gates are fused into its two loads), the gradient of ``postgate`` from one forward
    launch recomputed without it.  Modes "same" and "valid" first zero-embed the incoming gradient into the window of the
    full result with one torch pad and then take the route of "full".  No double backward, no torch.compile / functorch
    rules.  Otherwise the result carries no grad_fn and the call is what it has always been.
    Plans are cached per (shape, dtype, n, mode, device, stream); the filter is transformed on every call, so loops over one
    filter should use ``plan_fftconv``.
    Rows too long for one FFT (L + K - 1 beyond fftconv_length's last length) run as overlap-save blocks of
    fftconv_block(K) points, in the same single launch; ``block=`` forces that path at the given FFT length for any L (it
    excludes ``n``), K <= block - 1.
    ``partition=`` opens the partitioned path for filters longer than half a block (K > 8193; float64 4097), the Hyena-style
    K = L beyond one FFT: an integer Q cuts the filter into ceil(K / Q) partitions of Q taps at ``block=`` (default: the largest
    power-of-two block, 16384 / float64 8192), 1 <= Q <= block - 1, for any K; "auto" takes the paths above whenever they
    exist (the same bits) and fftconv_partition(K) otherwise.  One launch, no intermediate; the work grows with K / Q
    (DESIGN.md 3.4q).  It excludes ``n``; None refuses such filters as ever.  Gates, skip and autograd as on the other paths
    (the filter gradient: the fused partitioned plan, ``FusedPartConvGradPlan``, where it was measured not slower --
    ``_FFTCONV_FUSED_GRAD``, or ``fftconv_fused_filter_grad`` around the call -- and otherwise one launch of the overlap-save
    filter-gradient plan per partition).
    ``pregate`` / ``postgate`` / ``skip`` make it the gated filter stage of Hyena / H3 / S4 models in the same launch:
    ``postgate * (conv(pregate * x, k) + skip * (pregate * x))``.  ``pregate`` has exactly ``x``'s shape, ``postgate`` exactly
    the result's (ValueError otherwise: nothing is broadcast, a gate broadcast and then copied would cost what the fusion
    saves); both live on ``x``'s device and are converted to the working dtype as ``x`` is.  ``skip`` is a float or a real (D,)
    tensor, one value per channel, added to every bin of the filter spectrum (the term costs no kernel work).
    ``io_dtype`` = torch.bfloat16 or torch.float16 is the half-precision route, on every path above: ``x`` and the gates are
    read as tensors of ``io_dtype`` (without a copy when they already are, converted otherwise), widened exactly in the
    kernel's load, the arithmetic and the filter spectrum are float32, and the result is rounded once (to nearest even) in
    the kernel's store and has ``io_dtype`` -- the bits of ``fftconv(x.float(), k.float(), ...).to(io_dtype)`` in the same
    single launch.  Half-precision callers (autocast) should pass ``io_dtype=x.dtype``: without it a bfloat16 / float16
    ``x`` is still converted to float64, as ever.  Autograd with ``io_dtype``: the gradient of ``x`` (and the pregate route)
    is one launch of the opposite-``correlate`` half-storage plan on the incoming gradient (converted to ``io_dtype`` if it
    arrives otherwise); the gradient of ``k`` and ``skip`` comes from the half-storage filter-gradient kernel on ``x`` and the
    incoming gradient directly; with gates the same kernel reads them too and forms the products pregate * x and
    postgate * gradient in float32 in its loads (widen, then multiply), so that no product is rounded to 16 bits and no
    float32 copy is made.  Every returned gradient has the dtype of its tensor."""
    if x.is_complex() or k.is_complex():
        raise MifftError(-3, "fftconv expects real tensors (complex rows are out of scope)")
    if mode not in _FFTCONV_MODES:
        raise ValueError(f"fftconv: mode must be one of {_FFTCONV_MODES}, got {mode!r}")
    if correlate and mode != "causal":
        raise ValueError(f"fftconv: correlate=True goes with mode='causal' only, got {mode!r}")
    if k.dim() not in (1, 2) or x.dim() < k.dim():
        raise MifftError(-1, f"fftconv expects x (..., D, L) with k (D, K), or x (..., L) with k (K,), got {tuple(x.shape)} "
                             f"and {tuple(k.shape)}")
    logical = tuple(x.shape)
    L, K = int(logical[-1]), int(k.shape[-1])
    D = int(k.shape[0]) if k.dim() == 2 else 1
    if k.dim() == 2 and logical[-2] != D:
        raise MifftError(-2, f"fftconv: x has {logical[-2]} channels, k has {D} filters")
    if L < 2 or K < 1:
        raise MifftError(-2, f"fftconv: rows of {L} samples (at least 2) and filters of {K} taps (at least 1)")
    if io_dtype is not None and io_dtype not in _IO_DTYPES:
        raise MifftError(-4, f"fftconv: io_dtype is torch.bfloat16 or torch.float16 (or None), got {io_dtype}")
    dtype, sdt = _fftconv_dtypes(x, io_dtype)
    n, taps, Q = _fftconv_pick_part("fftconv", L, K, dtype, n, block, partition)
    offset, out_length = _fftconv_window(mode, L, K)
    rows = math.prod(logical[:-1])
    if rows < 1:
        raise MifftError(-8, f"fftconv: no rows in {logical}")
    for g, shape, what, of in ((pregate, logical, "pregate", "x"), (postgate, logical[:-1] + (out_length,), "postgate", "the result")):
        if g is None:
            continue
        if g.is_complex():
            raise MifftError(-3, f"fftconv: {what} must be real")
        if tuple(g.shape) != shape:
            raise ValueError(f"fftconv: {what} is {tuple(g.shape)}, {of} is {shape}: a gate has exactly that shape (nothing is "
                             "broadcast: a gate broadcast and then copied would cost what the fusion saves)")
        if g.device != x.device:
            raise MifftError(-10, f"fftconv: {what} lives on {g.device}, x on {x.device}")
    if skip is not None:
        if isinstance(skip, torch.Tensor):
            if skip.is_complex() or tuple(skip.shape) != (D,):
                raise ValueError(f"fftconv: skip is a float or a real tensor of shape ({D},), one value per channel, got "
                                 f"{tuple(skip.shape)} {skip.dtype}")
        else:
            skip = float(skip)
    device = _signal_device(x, "x")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, k, pregate, postgate, skip)):
        # (the forward of the Function runs with grad mode off: it comes back here and takes the lines below)
        skip_t = skip if isinstance(skip, torch.Tensor) else None
        # (the selector's answer is taken here, on the caller's thread: the backward runs on autograd's)
        return _FFTConvFunction.apply(x, k, pregate, postgate, skip_t, None if skip_t is not None else skip,
                                      (n, taps, mode, bool(correlate), Q, io_dtype, _fftconv_grad_fused(None, sdt, n, K, Q)))
    xr = x.to(sdt).contiguous().reshape(rows, L, 1)
    out = torch.empty((rows, out_length, 1), dtype=sdt, device=xr.device)
    gates = (1 if pregate is not None else 0) | (2 if postgate is not None else 0)
    with _PLAN_CACHE_LOCK:
        plan = _fftconv_fwd_plan(dtype, rows, D, L, n, taps, offset, out_length, correlate, device, gates, Q, io_dtype)
        a = pregate.to(sdt).contiguous().reshape(rows, L, 1) if pregate is not None else None
        b = postgate.to(sdt).contiguous().reshape(rows, out_length, 1) if postgate is not None else None
        _fftconv_exec(plan, out, xr, k, skip, a, b)
    return out.reshape(logical[:-1] + (out_length,))


class ConvPairPlan(Plan):
    """The plan of ``plan_fftconv_pair``: one launch per exec, no scratch, no state between execs.  ``in_shape``
    (batch, length, 1) is x's, ``v_shape`` (batch, taps, 1) the second operand's, ``out_shape`` (batch, out_length, 1);
    ``x_offset`` / ``v_offset`` / ``offset`` / ``correlate`` as given.  Runs through ``run(out, x, v)``."""

    def __init__(self, dtype, batch, length, taps, n, x_offset, v_offset, offset, out_length, correlate, ctx):
        self.ctx = ctx
        self.length, self.taps, self.n = length, taps, n
        self.x_offset, self.v_offset, self.offset, self.out_length = x_offset, v_offset, offset, out_length
        self.correlate = bool(correlate)
        self.v_shape = (batch, taps, 1)
        super().__init__(dtype, dtype, (batch, length, 1), (batch, out_length, 1), device=ctx.device,
                         conv=ConvPairRequest(n, taps, x_offset, v_offset, offset, out_length, 1 if correlate else 0))

    def run(self, out: "torch.Tensor", x: "torch.Tensor", v: "torch.Tensor", *, first: Optional[int] = None,
            count: Optional[int] = None) -> None:
        """``out[r] = irfft(rfft(xe[r]) * G[r], n)[offset : offset + out_length]`` for the rows ``first`` .. ``first + count - 1``
        (default: all), enqueued on the plan's stream.  ``x`` of ``in_shape``, ``v`` of ``v_shape``, ``out`` of ``out_shape``, the
        plan's dtype, contiguous, on its device; all three are the WHOLE batch's, the library offsets them by ``first`` rows.
        ``x`` and ``v`` may be the same tensor; neither may overlap ``out``; neither is written.  No autograd."""
        _check_tensor(x, self.in_shape, self.in_dtype, self.device, "x")
        _check_tensor(v, self.v_shape, self.in_dtype, self.device, "v")
        _check_tensor(out, self.out_shape, self.out_dtype, self.device, "out")
        first = 0 if first is None else int(first)
        count = self.out_shape[0] - first if count is None else int(count)
        args = ConvPairArgs(CONV_PAIR_ARGS_MAGIC, x.data_ptr(), v.data_ptr())
        check(_lib.lib().mifft_exec_batch(self._h, ctypes.addressof(args), out.data_ptr(), first, count,
                                          self.ctx.stream.cuda_stream))


def plan_fftconv_pair(dtype, batch: int, length: int, taps: int, n: int, *, x_offset: int = 0, v_offset: int = 0,
                      offset: int = 0, out_length: Optional[int] = None, correlate: bool = False,
                      ctx: Optional[DeviceContext] = None) -> ConvPairPlan:
    """Plan of the FFT convolution / correlation of two signal batches (no reference counterpart; MIFFT_CONV_PAIR_TAG in
    include/mifft.h): ``batch`` rows of ``length`` samples against ``batch`` rows of ``taps`` samples, row by row, at the FFT
    length ``n`` (see fftconv_length), in ONE kernel launch with no spectrum in memory.  With xe = zeros(n),
    xe[x_offset : x_offset + length] = x[r] and ve likewise from ``v_offset`` on:
    ``out[r] = irfft(rfft(xe) * rfft(ve), n)[offset : offset + out_length]`` (``correlate``: times conj(rfft(ve)), that is
    y[t] = sum_j ve[j] xe[(t + j) mod n]).  ``out_length`` defaults to ``length``.  float32 / float64.  Every argument error is
    raised before any device work.  ``plan.run(out, x, v)``; no autograd at the plan level (``fftconv_pair`` has it)."""
    batch, length, taps, n = int(batch), int(length), int(taps), int(n)
    ea, eb, offset = int(x_offset), int(v_offset), int(offset)
    out_length = length if out_length is None else int(out_length)
    who = "plan_fftconv_pair"
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"a two-signal convolution plan reads and writes float32 or float64, got {dtype}")
    if batch < 1:
        raise MifftError(-8, f"{who}: batch = {batch} must be positive")
    _fftconv_check_length(who, "n", n, dtype)
    if length < 2 or taps < 1:
        raise MifftError(-2, f"{who}: rows of {length} samples (at least 2) against rows of {taps} samples (at least 1)")
    if ea < 0 or eb < 0 or ea + length > n or eb + taps > n:
        raise MifftError(-5, f"{who}: x_offset = {ea} with length = {length}, v_offset = {eb} with taps = {taps}: both rows lie "
                             f"inside the FFT length, 0 <= offset and offset + samples <= n = {n}")
    if offset < 0 or out_length < 1 or offset + out_length > n:
        raise MifftError(-5, f"{who}: offset = {offset}, out_length = {out_length}: 0 <= offset, 1 <= out_length, "
                             f"offset + out_length <= n = {n}")
    return ConvPairPlan(dtype, batch, length, taps, n, ea, eb, offset, out_length, correlate, DeviceContext() if ctx is None else ctx)


def _fftconv_pair_plan(dtype, rows, L, K, n, ea, eb, o, Lo, correlate, device) -> ConvPairPlan:
    """the cached plan of ``fftconv_pair`` and of its backward (the caller holds _PLAN_CACHE_LOCK)"""
    return _plan_cached(("fftconv_pair", dtype, rows, L, K, n, ea, eb, o, Lo, bool(correlate)), device, lambda: plan_fftconv_pair(
        dtype, rows, L, K, n, x_offset=ea, v_offset=eb, offset=o, out_length=Lo, correlate=correlate, ctx=DeviceContext(device)))


def _fftconv_pair_exec(dtype, a, b, n, ea, eb, o, Lo, correlate, device) -> "torch.Tensor":
    """one launch of the cached pair plan on the contiguous (rows, La) and (rows, Lb) tensors a and b: (rows, Lo)"""
    rows, La, Lb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    out = torch.empty((rows, Lo, 1), dtype=dtype, device=a.device)
    with _PLAN_CACHE_LOCK:
        plan = _fftconv_pair_plan(dtype, rows, La, Lb, n, ea, eb, o, Lo, correlate, device)
        plan.run(out, a.reshape(rows, La, 1), b.reshape(rows, Lb, 1))
    return out.reshape(rows, Lo)


def _fftconv_pair_call(x, v, n, mode, correlate) -> tuple:
    """the checks of ``fftconv_pair``, all before any device work: (dtype, logical shape of x, L, K, n, ea, eb, o, Lo)"""
    who = "fftconv_pair"
    if x.is_complex() or v.is_complex():
        raise MifftError(-3, f"{who} expects real tensors (complex rows are out of scope)")
    if mode not in _FFTCONV_MODES:
        raise ValueError(f"{who}: mode must be one of {_FFTCONV_MODES}, got {mode!r}")
    if x.dim() < 1 or v.dim() < 1 or tuple(x.shape[:-1]) != tuple(v.shape[:-1]):
        raise MifftError(-2, f"{who}: x is {tuple(x.shape)} and v is {tuple(v.shape)}: both operands are signals with exactly the "
                             "same leading shape, one row of v per row of x (nothing is broadcast: a filter shared by the rows is "
                             "fftconv's job)")
    logical = tuple(x.shape)
    L, K = int(logical[-1]), int(v.shape[-1])
    if L < 2 or K < 1:
        raise MifftError(-2, f"{who}: rows of {L} samples (at least 2) against rows of {K} samples (at least 1)")
    if math.prod(logical[:-1]) < 1:
        raise MifftError(-8, f"{who}: no rows in {logical}")
    dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    if n is None:
        try:
            n = fftconv_length(L + K - 1, dtype)
        except MifftError as e:
            if e.status != ERR_UNSUPPORTED:
                raise
            raise MifftError(ERR_UNSUPPORTED, f"{who}: rows of {L} and {K} samples need an FFT of {L + K - 1} points, beyond the "
                                              f"last packed length ({_FFTCONV_MAX}; float64 12288): one FFT per row is all this "
                                              "op has -- long rows against a shared filter live in fftconv(block=)") from None
    else:
        n = int(n)
        _fftconv_check_length(who, "n", n, dtype)
        if n < L + K - 1 and mode != "causal":
            raise MifftError(-2, f"{who}: n = {n} is shorter than the full result of {L + K - 1} samples: the circular result "
                                 f"goes with mode='causal' only, got {mode!r}")
        if n < max(L, K):
            raise MifftError(-2, f"{who}: n = {n} does not hold rows of {L} and {K} samples (n >= max(L, K))")
    ea, eb, o, Lo = _fftconv_pair_window(mode, L, K, bool(correlate))
    return dtype, logical, L, K, n, ea, eb, o, Lo


def fftconv_pair(x: "torch.Tensor", v: "torch.Tensor", *, n: Optional[int] = None, mode: str = "full",
                 correlate: bool = False) -> "torch.Tensor":
    """Convolution (``correlate=True``: cross-correlation) by FFT of two real signal batches along the last dim, row by row:
    ``x`` of shape (..., L) and ``v`` of shape (..., K) with exactly the same leading shape -- one row of ``v`` per row of
    ``x``; nothing is broadcast (a filter shared by the rows is ``fftconv``'s job).  ONE kernel launch: both rows are
    transformed in the kernel, multiplied, transformed back and cropped; no padded copy and no spectrum reaches memory.
    ``x is v`` is the autocorrelation.  The result is (..., Lo).
    Modes "full" / "same" / "valid" are scipy.signal.fftconvolve(x, v, mode) or, with ``correlate=True``,
    scipy.signal.correlate(x, v, mode); "causal" is the first L samples of the product with both rows at index 0 -- of a
    correlation the lags 0 .. L - 1, y[t] = sum_j v[j] x[t + j].
    ``n`` is the FFT length, default fftconv_length(L + K - 1); a smaller one (n >= max(L, K)) is accepted with
    ``mode="causal"`` only and gives the circular result.  Rows with L + K - 1 beyond the last packed length (16384; float64
    12288) are refused.  float32 / float64; other input is converted to float64.
    Differentiable, first order: when grad mode is on and ``x`` or ``v`` requires grad the call goes through a
    torch.autograd.Function whose forward is this same launch (the same bits) and whose backward computes only the gradients
    asked for, each by ONE launch of a cached plan of this same kind on the incoming gradient (made contiguous if it is not),
    without padding it.  No double backward.  Otherwise the result carries no grad_fn."""
    dtype, logical, L, K, n, ea, eb, o, Lo = _fftconv_pair_call(x, v, n, mode, correlate)
    device = _signal_device(x, "x")
    if v.device != x.device:
        raise MifftError(-10, f"fftconv_pair: v lives on {v.device}, x on {x.device}")
    if torch.is_grad_enabled() and (x.requires_grad or v.requires_grad):
        return _FFTConvPairFunction.apply(x, v, (n, mode, bool(correlate)))
    rows = math.prod(logical[:-1])
    xr = x.to(dtype).contiguous().reshape(rows, L)
    vr = xr if v is x else v.to(dtype).contiguous().reshape(rows, K)
    return _fftconv_pair_exec(dtype, xr, vr, n, ea, eb, o, Lo, correlate, device).reshape(logical[:-1] + (Lo,))


class _FFTConvPairFunction(torch.autograd.Function):
    """``fftconv_pair`` with a backward (first order).  forward: the plain call, grad mode off.  backward: the gradients asked
    for, one launch each of the pair plans of ``_fftconv_pair_adjoints`` on gy as it arrives."""

    @staticmethod
    def forward(ctx, x, v, cfg):
        n, mode, correlate = cfg
        ctx.cfg = cfg
        ctx.save_for_backward(x, v)
        return fftconv_pair(x, v, n=n, mode=mode, correlate=correlate)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, v = ctx.saved_tensors
        n, mode, correlate = ctx.cfg
        dtype, logical, L, K, n, ea, eb, o, Lo = _fftconv_pair_call(x, v, n, mode, correlate)
        rows = math.prod(logical[:-1])
        device = x.device.index
        gyr = gy.to(dtype).contiguous().reshape(rows, Lo)  # (sum().backward() hands in an expanded tensor)
        xr = x.detach().to(dtype).contiguous().reshape(rows, L)
        vr = v.detach().to(dtype).contiguous().reshape(rows, K)
        # (no plan has a first dimension of 1: a one-sample gy that is the first operand gets one of the zeros the embedding
        #  would add anyway, behind it, or in front of it at the last index of the FFT length)
        front = Lo < 2 and o + 2 > n
        gy2 = gyr if Lo >= 2 else torch.nn.functional.pad(gyr, (1, 0) if front else (0, 1))
        grads = []
        for need, other, (first, La, Lb, a_e, b_e, a_o, a_Lo, a_corr) in zip(
                ctx.needs_input_grad[:2], (vr, xr), _fftconv_pair_adjoints(L, K, ea, eb, o, Lo, correlate)):
            if not need:
                grads.append(None)
                continue
            a, b = (gy2, other) if first == "gy" else (other, gyr)
            if first == "gy" and front:
                a_e -= 1
            g = _fftconv_pair_exec(dtype, a, b, n, a_e, b_e, a_o, a_Lo, a_corr, device)
            grads.append(g)
        gx, gv = grads
        back = lambda g, t: None if g is None else g.reshape(t.shape).to(t.dtype)
        return back(gx, x), back(gv, v), None


class ConvGradPlan(Plan):
    """The plan of ``plan_fftconv_grad``: the filter gradient of the ``plan_fftconv`` plan of the same arguments, one launch
    of ``channels * partials`` persistent workgroups (MIFFT_CONV_GRAD_TAG in include/mifft.h).  ``partials`` partial sums
    per channel (the library's choice unless given), ``blocks`` per row and ``step`` samples per block as on ``ConvPlan``
    (a single block: 1 and None).  ``in_shape`` (batch * channels, length, 1) is x's, ``grad_shape``
    (batch * channels, out_length, 1) the incoming gradient's, ``out_shape`` (partials, channels, n // 2 + 1, 2).
    With ``io_dtype`` (torch.bfloat16 / torch.float16 under float32) ``x`` and ``gy`` are tensors of it, widened exactly in
    the kernel's loads; the result stays float32.  None on every other plan.
    A gated plan (``plan_fftconv_grad(pregate=True)`` and / or ``postgate=True``) has ``pregate`` / ``postgate`` True: it is
    the filter gradient of the gated forward plan, and ``run`` / ``filter_grad`` take the gate tensors of that exec, which
    the kernel multiplies into its loads of ``x`` and ``gy`` -- the bits of the ungated plan on the torch products
    ``pregate * x`` and ``postgate * gy``, in the same single launch and grid, without the products in memory."""

    def __init__(self, dtype, batch, channels, length, n, offset, out_length, correlate, ctx, taps=None, partials=None,
                 io_dtype=None, pregate=False, postgate=False):
        self.ctx = ctx
        self.io_dtype = io_dtype
        self.pregate, self.postgate = bool(pregate), bool(postgate)
        self.channels, self.length, self.n = channels, length, n
        self.offset, self.out_length, self.correlate = offset, out_length, bool(correlate)
        req = _fftconv_request(n, channels, offset, out_length, correlate, taps, None, io_dtype)
        self.taps, self.step, self.blocks = taps, req.S or None, req.F
        rows = batch * channels
        super().__init__(dtype, dtype, (rows, length, 1), (rows, out_length, 1), device=ctx.device,
                         conv=req._replace(grad=True, partials=0 if partials is None else int(partials),
                                           gates=(1 if self.pregate else 0) | (2 if self.postgate else 0)))
        self.grad_shape = self.out_shape  # (what Plan takes for the other side of x; the result's shape needs the built plan)
        self.partials = self.pass_geometry(1)[3] // channels
        self.out_shape = (self.partials, channels, n // 2 + 1, 2)

    def pass_geometry(self, dim: int, count: Optional[int] = None) -> tuple:
        """(tile, threads, n_tiles, grid): pairs per step of a workgroup, threads, the steps of all workgroups, and
        ``channels * partials`` workgroups; workgroup (d, p) walks ceil(its pairs / tile) steps"""
        return super().pass_geometry(dim, self.in_shape[0] if count is None else count)

    def run(self, out: "torch.Tensor", x: "torch.Tensor", gy: "torch.Tensor", *, pregate: Optional["torch.Tensor"] = None,
            postgate: Optional["torch.Tensor"] = None) -> None:
        """fills ``out`` of ``out_shape`` with the unscaled partial spectra sum conj(rfft(x-block)) rfft(gy-block), enqueued on
        the plan's stream; ``x`` of ``in_shape`` and ``gy`` of ``grad_shape``, the plan's dtype (``io_dtype`` where it has one),
        contiguous; neither is written.  On a gated plan ``pregate`` of ``in_shape`` multiplies ``x`` and ``postgate`` of
        ``grad_shape`` multiplies ``gy`` as the kernel loads them, both of the dtype of ``x``, each given exactly where the
        plan has it (status -12 for a missing one, ERR_UNSUPPORTED for one the plan has none of).  A gate may alias ``x``,
        ``gy`` or the other gate, not ``out``."""
        for t, want, what in ((pregate, self.pregate, "pregate"), (postgate, self.postgate, "postgate")):
            if want and t is None:
                raise MifftError(-12, f"the plan has a {what}: run(..., {what}=) is missing")
            if not want and t is not None:
                raise MifftError(ERR_UNSUPPORTED, f"the plan has no {what}: plan_fftconv_grad(..., {what}=True) makes one that has")
        sdt = self.io_dtype or self.in_dtype
        _check_tensor(x, self.in_shape, sdt, self.device, "x")
        _check_tensor(gy, self.grad_shape, sdt, self.device, "gy")
        if pregate is not None:
            _check_tensor(pregate, self.in_shape, sdt, self.device, "pregate")
        if postgate is not None:
            _check_tensor(postgate, self.grad_shape, sdt, self.device, "postgate")
        _check_tensor(out, self.out_shape, self.out_dtype, self.device, "out")
        if self.conv_gates:
            args = ConvGradGatedArgs(CONV_GRAD_GATED_ARGS_MAGIC, x.data_ptr(), gy.data_ptr(),
                                     pregate.data_ptr() if pregate is not None else None,
                                     postgate.data_ptr() if postgate is not None else None)
        else:
            args = ConvGradArgs(CONV_GRAD_ARGS_MAGIC, x.data_ptr(), gy.data_ptr())
        check(_lib.lib().mifft_exec_batch(self._h, ctypes.addressof(args), out.data_ptr(), 0, self.in_shape[0],
                                          self.ctx.stream.cuda_stream))

    def filter_grad(self, x: "torch.Tensor", gy: "torch.Tensor", K: int, *, pregate: Optional["torch.Tensor"] = None,
                    postgate: Optional["torch.Tensor"] = None) -> "torch.Tensor":
        """the real (channels, K) gradient of the filter: ``run`` (with the gates of a gated plan), the sum of the partials,
        the library's own irfftn, the first K lags (lag 0 is also the gradient of a skip term)"""
        K = int(K)
        if K < 1 or K > self.n or (self.taps is not None and K > self.taps):
            raise MifftError(-2, f"filter_grad: K = {K} taps at n = {self.n}" +
                                 (f" on an overlap-save plan of taps = {self.taps}" if self.taps is not None else "") +
                                 ": 1 <= K <= " + str(self.n if self.taps is None else self.taps))
        out = torch.empty(self.out_shape, dtype=self.out_dtype, device=x.device)
        self.run(out, x, gy, pregate=pregate, postgate=postgate)
        with torch.cuda.stream(self.ctx.stream):
            A = out[0] if self.partials == 1 else out.sum(0)
            return irfftn(A, self.n)[:, :K]


class PartConvGradPlan:
    """The plan of ``plan_fftconv_grad(partition=Q)``: the filter gradient of the partitioned ``plan_fftconv`` plan of the same
    arguments, COMPOSED of one overlap-save filter-gradient plan (``ConvGradPlan``, taps = Q at the same block length) per
    partition -- ``partitions`` launches, not one.  Taps p Q .. (p + 1) Q - 1 of the gradient are the gradient of a filter of Q
    taps against the same rows with the window moved by p Q samples: ``gk[p Q + j] = sum_t gy[t] u[o - p Q + t - j]``
    (correlation: ``u[o + p Q + t + j]``), which is the existing plan on a contiguous slice of ``u`` (correlation) or of ``gy``
    (where o - p Q is negative), cropped to the samples that can meet.  ``plans[p]`` is None where none can: those taps are
    exact zeros.  Every sub-plan sums in an order fixed by its own shape, so two runs give the same bits.
    ``pregate`` / ``postgate`` are passed on to every sub-plan, which fuses them into its loads; the gate tensors are sliced as
    ``x`` and ``gy`` are.  Still composed, one launch per partition."""

    def __init__(self, dtype, batch, channels, length, n, offset, out_length, correlate, ctx, taps, partition, partials=None,
                 io_dtype=None, pregate=False, postgate=False):
        self.ctx, self.dtype, self.io_dtype = ctx, dtype, io_dtype  # (io_dtype: of x and gy, as on every ConvGradPlan below)
        self.pregate, self.postgate = bool(pregate), bool(postgate)
        self.channels, self.length, self.n = channels, length, n
        self.offset, self.out_length, self.correlate = offset, out_length, bool(correlate)
        self.taps, self.partition, self.partitions = taps, partition, -(-taps // partition)
        self.step = n - partition + 1
        rows = batch * channels
        self.in_shape, self.grad_shape = (rows, length, 1), (rows, out_length, 1)
        self.device = int(ctx.device)
        self.slices = [_fftconv_part_grad_slice(length, partition, offset, out_length, correlate, p) for p in range(self.partitions)]
        self.plans = [None if sl is None else
                      plan_fftconv_grad(dtype, batch, channels, max(sl[1] - sl[0], 2), n, taps=partition, offset=sl[4],
                                        out_length=sl[3] - sl[2], correlate=correlate, partials=partials, ctx=ctx,
                                        io_dtype=io_dtype, pregate=self.pregate, postgate=self.postgate)
                      for sl in self.slices]

    @property
    def num_launches(self) -> int:
        return sum(pl.num_launches for pl in self.plans if pl is not None)

    @property
    def scratch_bytes(self) -> int:
        return sum(pl.scratch_bytes for pl in self.plans if pl is not None)

    def close(self) -> None:
        for pl in self.plans:
            if pl is not None:
                pl.close()

    def filter_grad(self, x: "torch.Tensor", gy: "torch.Tensor", K: int, *, pregate: Optional["torch.Tensor"] = None,
                    postgate: Optional["torch.Tensor"] = None) -> "torch.Tensor":
        """the real (channels, K) gradient of the filter, K <= taps: ``ConvGradPlan.filter_grad`` of every partition on its
        slices of ``x`` of ``in_shape`` and ``gy`` of ``grad_shape`` (copied where they are no whole rows), concatenated.
        On a gated plan ``pregate`` of ``in_shape`` and ``postgate`` of ``grad_shape`` are sliced as ``x`` and ``gy`` are."""
        K = int(K)
        if K < 1 or K > self.taps:
            raise MifftError(-2, f"filter_grad: K = {K} taps on a partitioned plan of taps = {self.taps}: 1 <= K <= {self.taps}")
        for t, want, what in ((pregate, self.pregate, "pregate"), (postgate, self.postgate, "postgate")):
            if want and t is None:
                raise MifftError(-12, f"the plan has a {what}: filter_grad(..., {what}=) is missing")
            if not want and t is not None:
                raise MifftError(ERR_UNSUPPORTED, f"the plan has no {what}: plan_fftconv_grad(..., {what}=True) makes one that has")
        _check_tensor(x, self.in_shape, self.io_dtype or self.dtype, self.device, "x")
        _check_tensor(gy, self.grad_shape, self.io_dtype or self.dtype, self.device, "gy")
        if pregate is not None:
            _check_tensor(pregate, self.in_shape, self.io_dtype or self.dtype, self.device, "pregate")
        if postgate is not None:
            _check_tensor(postgate, self.grad_shape, self.io_dtype or self.dtype, self.device, "postgate")
        Q, parts = self.partition, []
        with torch.cuda.stream(self.ctx.stream):
            for p in range(-(-K // Q)):
                Kp = min(Q, K - p * Q)
                sl, plan = self.slices[p], self.plans[p]
                if plan is None:
                    parts.append(torch.zeros((self.channels, Kp), dtype=self.dtype, device=x.device))
                    continue
                us, gs, pa, pb = _fftconv_part_grad_operands(sl, x, gy, pregate, postgate)
                parts.append(plan.filter_grad(us, gs, Kp, pregate=pa, postgate=pb))
            return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _fftconv_part_grad_operands(sl: tuple, x, gy, pregate=None, postgate=None) -> tuple:
    """(us, gs, a, b), contiguous: what partition ``sl`` = (u0, u1, g0, g1, offset) of the composed filter gradient reads of
    ``x`` (rows, L, 1) and ``gy`` (rows, Lo, 1) -- x[:, u0:u1], padded to rows of two samples, and gy[:, g0:g1] -- and of the
    gates, the pregate sliced and padded exactly as ``x``, the postgate sliced exactly as ``gy`` (None stays None)"""
    u0, u1, g0, g1, _ = sl

    def of_x(t):
        t = t[:, u0:u1]
        if u1 - u0 < 2:  # (rows of at least two samples: a zero behind the one)
            t = torch.nn.functional.pad(t, (0, 0, 0, 2 - (u1 - u0)))
        return t.contiguous()

    return (of_x(x), gy[:, g0:g1].contiguous(), None if pregate is None else of_x(pregate),
            None if postgate is None else postgate[:, g0:g1].contiguous())


def _fftconv_part_grad_slice(L: int, Q: int, o: int, Lo: int, correlate: bool, p: int):
    """(u0, u1, g0, g1, offset) of partition p of the composed filter gradient: the overlap-save filter-gradient plan of Q taps
    and that offset on u[u0:u1] and gy[g0:g1] gives the taps p Q .. of the filter gradient; None when no sample of gy meets a
    sample of u (the taps are zero)."""
    if correlate:  # gk[p Q + j] = sum_t gy[t] u[p Q + o + t + j]: u from p Q on, gy as far as it reaches into it
        u0, u1 = p * Q, L
        g1 = min(Lo, u1 - u0 - o)
        return None if u1 - u0 < 1 or g1 < 1 else (u0, u1, 0, g1, o)
    off = o - p * Q  # gk[p Q + j] = sum_t gy[t] u[off + t - j]
    if off >= 0:
        g1 = min(Lo, L + Q - 1 - off)
        return None if g1 < 1 else (0, L, 0, g1, off)
    g0 = -off  # (earlier samples of gy meet u before its first sample); gy' = gy[g0:] at offset 0, u as far as gy' reaches
    if g0 >= Lo:
        return None
    g1 = min(Lo, g0 + L + Q - 1)
    return (0, min(L, g1 - g0), g0, g1, 0)


class FusedGradGeometry(NamedTuple):
    """The geometry of the fused partitioned filter gradient (``_fftconv_fused_grad_geometry``; mirrored by the payload
    decode of the library, include/mifft.h): ``H`` = n // 2 samples per step and lags per group, ``Pg`` lag groups, ``Fg``
    g-blocks, ``c`` the index of a g-block's first sample (H, correlating 0), the u-frames ``m_lo`` .. ``m_hi`` the sums name,
    the live ones among them ``u_first`` .. ``u_first + Fu - 1`` (``Fu`` = 0: none) and ``u_start``, the first sample of frame
    ``u_first``.  ``frame_start(m)`` is the first sample of u-frame m, ``lag_frame(f, p)`` the frame (g-block f, lag group p)
    meets, ``reachable`` the taps (j0, j1) -- j0 <= j < j1 -- that any pair of samples can reach."""
    n: int
    H: int
    Pg: int
    Fg: int
    c: int
    m_lo: int
    m_hi: int
    u_first: int
    Fu: int
    u_start: int
    correlate: bool
    offset: int
    reachable: tuple

    def frame_start(self, m: int) -> int:
        return self.offset + m * self.H - (0 if self.correlate else self.H)

    def lag_frame(self, f: int, p: int) -> int:
        return f + p if self.correlate else f - p

    def live(self, m: int) -> bool:
        return self.u_first <= m < self.u_first + self.Fu


def _fftconv_fused_grad_geometry(n: int, L: int, Lo: int, K: int, o: int, correlate: bool) -> FusedGradGeometry:
    """The one host function of the fused partitioned filter gradient's geometry: with H = n // 2, g-block f holds
    gv[f H + i], i < H, at index c + i; u-frame m is the n samples of u from o + m H - H on (correlating: o + m H), zeros
    outside [0, L); lag group p of g-block f meets frame f - p (correlating: f + p).  A frame that holds no sample of [0, L)
    is dead: neither transformed nor stored.  Pure: no device, no library call."""
    n, L, Lo, K, o, correlate = int(n), int(L), int(Lo), int(K), int(o), bool(correlate)
    H = n // 2
    Pg, Fg = -(-K // H), -(-Lo // H)
    m_lo, m_hi = (0, Fg + Pg - 2) if correlate else (-(Pg - 1), Fg - 1)
    base = o if correlate else o - H  # (the first sample of frame 0)
    # live: base + m H > -n and base + m H < L
    first = max(m_lo, (-n - base) // H + 1)
    last = min(m_hi, -(-(L - base) // H) - 1)
    Fu = max(0, last - first + 1)
    # tap j meets a pair of samples for some t in [0, Lo): 0 <= o + t - j < L (correlating: o + t + j < L)
    reach = (0, max(0, min(K, L - o))) if correlate else (max(0, o - L + 1), max(0, min(K, o + Lo)))
    return FusedGradGeometry(n, H, Pg, Fg, 0 if correlate else H, m_lo, m_hi, first, Fu, base + first * H, correlate, o, reach)


# stage 2 reads what stage 1 just wrote from the memory-side cache while both spectra tensors of a slab, and the rows stage 1
# streams past them, stay inside it: half the Infinity Cache (kInfinityCacheBytes, csrc/mifft_config.h) for the spectra
_INFINITY_CACHE_BYTES = 256 << 20
_FUSED_GRAD_SCRATCH_DEFAULT = _INFINITY_CACHE_BYTES // 2
_FUSED_GRAD_MAX_LAG_GROUPS = 32


def _fftconv_fused_grad_entry_bytes(g: FusedGradGeometry, channels: int, dtype) -> int:
    """the bytes of the two spectra tensors of ONE batch entry: channels (Fu + Fg) (n // 2 + 1) complex values of ``dtype``"""
    return int(channels) * (g.Fu + g.Fg) * (g.n // 2 + 1) * 2 * (8 if dtype == torch.float64 else 4)


def _fftconv_fused_grad_slabs(batch: int, entry_bytes: int, limit: Optional[int]) -> list:
    """The slabs [(b0, b1), ..] of the fused partitioned filter gradient: whole batch entries, ascending, covering the batch
    once, each of at most ``limit`` bytes of spectra, the fewest such slabs, their sizes differing by one entry at most (the
    larger first).  ``limit`` None is the default, ``_FUSED_GRAD_SCRATCH_DEFAULT`` -- or one entry where that alone is larger,
    so the default never refuses.  MifftError(ERR_UNSUPPORTED) when a given limit does not hold one entry."""
    batch, entry_bytes = int(batch), int(entry_bytes)
    if limit is None:
        limit = max(_FUSED_GRAD_SCRATCH_DEFAULT, entry_bytes)
    limit = int(limit)
    if entry_bytes > limit:
        raise MifftError(ERR_UNSUPPORTED, f"plan_fftconv_grad(fused=True): the spectra of one batch entry take {entry_bytes} bytes, "
                                          f"above scratch_bytes = {limit}; the composed per-partition plan (fused=False) needs "
                                          "no scratch")
    per = max(1, limit // max(entry_bytes, 1))
    count = -(-batch // per)
    small, extra = divmod(batch, count)
    out, b = [], 0
    for i in range(count):
        size = small + (1 if i < extra else 0)
        out.append((b, b + size))
        b += size
    return out


class _ConvGradStagePlan(Plan):
    """one stage of a ``FusedPartConvGradPlan``: a filter-gradient plan whose payload names a stage (ConvRequest.stage)"""

    def __init__(self, dtype, in_shape, out_shape, ctx, req: ConvRequest, io_dtype=None):
        self.ctx, self.io_dtype = ctx, io_dtype
        super().__init__(dtype, dtype, in_shape, out_shape, device=ctx.device, conv=req)

    def launch(self, out: "torch.Tensor", x, gy, pregate=None, postgate=None) -> None:
        """``x`` / ``gy`` / the gates: device addresses (None where the stage reads none)"""
        if self.conv_gates:
            args = ConvGradGatedArgs(CONV_GRAD_GATED_ARGS_MAGIC, x, gy, pregate, postgate)
        else:
            args = ConvGradArgs(CONV_GRAD_ARGS_MAGIC, x, gy)
        check(_lib.lib().mifft_exec_batch(self._h, ctypes.addressof(args), out.data_ptr(), 0, self.in_shape[0],
                                          self.ctx.stream.cuda_stream))


class FusedPartConvGradPlan:
    """The plan of ``plan_fftconv_grad(partition=Q, fused=True)``: the filter gradient of the partitioned ``plan_fftconv`` plan
    of the same arguments with every block of ``u`` and of ``gy`` transformed ONCE -- a frequency-domain delay line -- where
    ``PartConvGradPlan`` transforms them again for every partition.  The gradient of a linear convolution is the
    cross-correlation ``gk[j] = sum_t gy[t] u[o + t - j]`` whatever Q the forward chose, so the plan takes its own step
    ``hop`` = n // 2 and ``lag_groups`` = ceil(taps / hop) groups of ``hop`` lags (``_fftconv_fused_grad_geometry``):
    stage 1 stores the half spectra of the live u-frames and of the g-blocks (the filter-gradient tile's two loads, gates and
    16-bit widening included: TileCfg::WSPEC), stage 2 (lag_corr.hip) sums ``conj(U[f - p]) G[f]`` over the batch and the
    blocks for every lag group p, and one ``irfftn`` of ``channels * lag_groups`` rows gives the taps.
    The spectra live in plan-owned scratch, ``scratch_bytes`` in all (what was allocated): the batch is cut into ``slabs`` of
    whole entries whose spectra stay under the limit (``scratch_bytes=``; default half the Infinity Cache, so that stage 2
    reads from the cache what stage 1 wrote), three launches and one partial per slab; the partials are summed in ascending
    order.  Every sum runs in an order the plan fixes: two runs, or two plans of the same arguments, give the same bits.
    ``partition`` / ``partitions`` / ``step`` describe the forward plan, as on ``PartConvGradPlan``.  Limits: ``lag_groups`` <=
    32 (ERR_UNSUPPORTED beyond, as for one batch entry above a given ``scratch_bytes``: the composed plan takes those), first
    order only, no fused gradient of the gates themselves."""

    def __init__(self, dtype, batch, channels, length, n, offset, out_length, correlate, ctx, taps, partition, io_dtype=None,
                 pregate=False, postgate=False, scratch_bytes=None):
        self.ctx, self.dtype, self.io_dtype = ctx, dtype, io_dtype
        self.pregate, self.postgate = bool(pregate), bool(postgate)
        self.channels, self.length, self.n = channels, length, n
        self.offset, self.out_length, self.correlate = offset, out_length, bool(correlate)
        self.taps, self.partition, self.partitions = taps, partition, -(-taps // partition)
        self.step = n - partition + 1
        self.batch = batch
        rows = batch * channels
        self.in_shape, self.grad_shape = (rows, length, 1), (rows, out_length, 1)
        self.device = int(ctx.device)
        g = self.geometry = _fftconv_fused_grad_geometry(n, length, out_length, taps, offset, correlate)
        self.hop, self.lag_groups = g.H, g.Pg
        if g.Pg > _FUSED_GRAD_MAX_LAG_GROUPS:
            raise MifftError(ERR_UNSUPPORTED, f"plan_fftconv_grad(fused=True): taps = {taps} at n = {n} are {g.Pg} lag groups of "
                                              f"{g.H}, above {_FUSED_GRAD_MAX_LAG_GROUPS}; the composed per-partition plan "
                                              "(fused=False) has no such limit")
        self.entry_bytes = _fftconv_fused_grad_entry_bytes(g, channels, dtype)
        self.slabs = _fftconv_fused_grad_slabs(batch, self.entry_bytes, scratch_bytes)
        self._stages, self._U, self._G, self.partials = {}, None, None, 0
        if g.Fu == 0:  # (no sample of gy meets a sample of u: every tap is an exact zero)
            self.slabs = []
            return
        bins, mode = n // 2 + 1, 1 if correlate else 0
        gates = (1 if self.pregate else 0) | (2 if self.postgate else 0)
        for b0, b1 in self.slabs:
            r = (b1 - b0) * channels
            if r in self._stages:
                continue
            up = _ConvGradStagePlan(dtype, (r, length, 1), (r, g.Fu * g.H, 1), ctx, ConvRequest(
                n, channels, 0, g.Fu * g.H, S=g.H, F=g.Fu, s0=g.u_start, mode=mode | _io_mode_bits(io_dtype), grad=True,
                gates=gates & 1, stage=1), io_dtype)
            gp = _ConvGradStagePlan(dtype, (r, max(out_length, 2), 1), (r, out_length, 1), ctx, ConvRequest(
                n, channels, g.c, out_length, S=g.H, F=g.Fg, s0=0, mode=mode | _io_mode_bits(io_dtype), grad=True,
                gates=gates & 2, stage=2), io_dtype)
            lp = _ConvGradStagePlan(dtype, (r, max(g.Fu, 2), 1), (r, g.Fg, 1), ctx, ConvRequest(
                n, channels, g.Fu, g.Fg, S=g.Pg, F=g.Fg, s0=g.u_first, mode=mode, grad=True, stage=3))
            lp.partials = lp.out_bytes // (channels * g.Pg * bins * 2 * (8 if dtype == torch.float64 else 4))
            self._stages[r] = (up, gp, lp)
        self.partials = sum(self._stages[(b1 - b0) * channels][2].partials for b0, b1 in self.slabs)
        most = max(b1 - b0 for b0, b1 in self.slabs) * channels
        with torch.cuda.stream(ctx.stream):
            self._U = torch.empty((most, g.Fu, bins, 2), dtype=dtype, device=f"cuda:{ctx.device}")
            self._G = torch.empty((most, g.Fg, bins, 2), dtype=dtype, device=f"cuda:{ctx.device}")

    @property
    def plans(self) -> list:
        """the (u-spectra, g-spectra, lag-group) plans of every slab, in slab order"""
        return [self._stages[(b1 - b0) * self.channels] for b0, b1 in self.slabs]

    @property
    def num_launches(self) -> int:
        return sum(sum(pl.num_launches for pl in trio) for trio in self.plans)

    @property
    def scratch_bytes(self) -> int:
        return 0 if self._U is None else (self._U.numel() * self._U.element_size() + self._G.numel() * self._G.element_size())

    def close(self) -> None:
        for trio in self._stages.values():
            for pl in trio:
                pl.close()
        self._stages, self._U, self._G, self.slabs = {}, None, None, []

    def spectra(self, x: "torch.Tensor", gy: "torch.Tensor", slab: int = 0, *, pregate=None, postgate=None) -> tuple:
        """stage 1 alone on slab ``slab``: (U, G), views of the plan's scratch -- complex (rows of the slab, Fu, n // 2 + 1) and
        (.., Fg, n // 2 + 1), stored frame j of U being u-frame ``geometry.u_first`` + j -- valid until the next call"""
        self._check(x, gy, pregate, postgate)
        b0, b1 = self.slabs[slab]
        with torch.cuda.stream(self.ctx.stream):
            U, G = self._stage1(x, gy, pregate, postgate, b0, b1)
        return torch.view_as_complex(U), torch.view_as_complex(G)

    def _check(self, x, gy, pregate, postgate) -> None:
        for t, want, what in ((pregate, self.pregate, "pregate"), (postgate, self.postgate, "postgate")):
            if want and t is None:
                raise MifftError(-12, f"the plan has a {what}: filter_grad(..., {what}=) is missing")
            if not want and t is not None:
                raise MifftError(ERR_UNSUPPORTED, f"the plan has no {what}: plan_fftconv_grad(..., {what}=True) makes one that has")
        sdt = self.io_dtype or self.dtype
        _check_tensor(x, self.in_shape, sdt, self.device, "x")
        _check_tensor(gy, self.grad_shape, sdt, self.device, "gy")
        if pregate is not None:
            _check_tensor(pregate, self.in_shape, sdt, self.device, "pregate")
        if postgate is not None:
            _check_tensor(postgate, self.grad_shape, sdt, self.device, "postgate")

    def _stage1(self, x, gy, pregate, postgate, b0: int, b1: int) -> tuple:
        r0, r = b0 * self.channels, (b1 - b0) * self.channels
        up, gp, _ = self._stages[r]
        U, G = self._U[:r], self._G[:r]
        xb, gb = x.element_size() * self.length, gy.element_size() * self.out_length  # (bytes per row)
        up.launch(U, x.data_ptr() + r0 * xb, None, None if pregate is None else pregate.data_ptr() + r0 * xb, None)
        gp.launch(G, None, gy.data_ptr() + r0 * gb, None, None if postgate is None else postgate.data_ptr() + r0 * gb)
        return U, G

    def filter_grad(self, x: "torch.Tensor", gy: "torch.Tensor", K: int, *, pregate: Optional["torch.Tensor"] = None,
                    postgate: Optional["torch.Tensor"] = None) -> "torch.Tensor":
        """the real (channels, K) gradient of the filter, K <= taps, from ``x`` of ``in_shape`` and ``gy`` of ``grad_shape``
        (on a gated plan with ``pregate`` of ``in_shape`` and ``postgate`` of ``grad_shape``, fused into stage 1's loads):
        per slab the two spectra launches and the lag-group launch, then the sum of the partials in ascending order, one
        ``irfftn`` and the first ``hop`` lags of every group.  Taps that no pair of samples can reach are exact zeros."""
        K = int(K)
        if K < 1 or K > self.taps:
            raise MifftError(-2, f"filter_grad: K = {K} taps on a partitioned plan of taps = {self.taps}: 1 <= K <= {self.taps}")
        self._check(x, gy, pregate, postgate)
        g, D = self.geometry, self.channels
        with torch.cuda.stream(self.ctx.stream):
            if g.Fu == 0:
                return torch.zeros((D, K), dtype=self.dtype, device=x.device)
            out = torch.empty((self.partials, D, g.Pg, self.n // 2 + 1, 2), dtype=self.dtype, device=x.device)
            at = 0
            for b0, b1 in self.slabs:
                U, G = self._stage1(x, gy, pregate, postgate, b0, b1)
                lp = self._stages[(b1 - b0) * D][2]
                lp.launch(out[at:at + lp.partials], U.data_ptr(), G.data_ptr())
                at += lp.partials
            A = out[0] if self.partials == 1 else out.sum(0)
            gk = irfftn(A.reshape(D * g.Pg, self.n // 2 + 1, 2), self.n).reshape(D, g.Pg, self.n)[:, :, :g.H]
            gk = gk.reshape(D, g.Pg * g.H)[:, :K].contiguous()
            j0, j1 = g.reachable
            if j0 > 0:
                gk[:, :min(j0, K)] = 0
            if j1 < K:
                gk[:, j1:] = 0
            return gk


# Where the fused partitioned filter gradient is taken by default (``fused=None``): {storage dtype: {n: least lag groups}},
# the keys at which profiles/r26_fftconv_part_grad.txt (tools/fftconv_part_grad_probe.py) shows its median
# not above the composed plan's beyond the spread of the composed plan's own windows, at every shape measured for the key.
# Every (dtype, n) that was not measured keeps the composed plan.
_FFTCONV_FUSED_GRAD = {
    torch.float32: {16384: 4},   # 4 x 256 x 32768, 4 x 256 x 65536, 4 x 64 x 131072: 0.59, 0.34 and 0.17 of the composed plan
    torch.float64: {8192: 8},    # 4 x 64 x 32768: 0.38
    torch.bfloat16: {16384: 8},  # 4 x 256 x 65536 with both gates: 0.34
}

_fused_grad_override = threading.local()


@contextlib.contextmanager
def fftconv_fused_filter_grad(fused: Optional[bool]):
    """Within the block, ``fftconv_filter_grad(fused=None)`` and every ``fftconv`` call on a partitioned path -- for its backward,
    whenever that runs -- take the fused partitioned filter gradient (True), the composed one (False) or the measured default
    (None), on this thread."""
    before = getattr(_fused_grad_override, "value", None)
    _fused_grad_override.value = fused
    try:
        yield
    finally:
        _fused_grad_override.value = before


def _fftconv_grad_fused(fused: Optional[bool], sdt, n: int, K: int, Q) -> bool:
    """The one selector of the partitioned filter gradient: does (storage dtype, block length, taps) take the fused plan?
    ``fused`` True / False is the caller's word (True off the partitioned path is an error), None the override of
    ``fftconv_fused_filter_grad`` and then the table ``_FFTCONV_FUSED_GRAD``."""
    if fused and Q is None:
        raise MifftError(-2, "fused=True is the fused gradient of the PARTITIONED path: it goes with partition=")
    if Q is None:
        return False
    if fused is None:
        fused = getattr(_fused_grad_override, "value", None)
    if fused is None:
        least = _FFTCONV_FUSED_GRAD.get(sdt, {}).get(int(n))
        lags = -(-int(K) // (int(n) // 2))
        return least is not None and least <= lags <= _FUSED_GRAD_MAX_LAG_GROUPS
    return bool(fused)


def plan_fftconv_grad(dtype, batch: int, channels: int, length: int, n: int, *, taps: Optional[int] = None, offset: int = 0,
                      out_length: Optional[int] = None, correlate: bool = False, partials: Optional[int] = None,
                      ctx: Optional[DeviceContext] = None, partition: Optional[int] = None, io_dtype=None,
                      pregate: bool = False, postgate: bool = False, fused: bool = False, scratch_bytes: Optional[int] = None):
    """Plan of the fused filter gradient (no reference counterpart) of the ``plan_fftconv`` plan of the same arguments:
    ``gk[d, j] = sum over b and t of gy[b, d, t] * u[b, d, o + t - j]`` (``correlate``: ``o + t + j``), computed as
    ``irfft(sum_b conj(rfft(u[b, d], n)) * rfft(gy[b, d] put at o, n), n)[:K]`` in ONE launch that reads ``u`` and ``gy`` once
    each and writes ``channels * partials`` rows of n // 2 + 1 bins -- the exact adjoint of what the forward plan computes,
    circular where that is, block by block on an overlap-save plan (``taps=K``).  ``partition=Q`` (with ``taps=K``, any K >= 1)
    gives the gradient of the partitioned plan as a ``PartConvGradPlan``: one such launch per partition -- or, with ``fused=True``,
    as a ``FusedPartConvGradPlan`` that transforms every block once (spectra in scratch bounded by ``scratch_bytes=``, default
    half the Infinity Cache; ERR_UNSUPPORTED above 32 lag groups of n // 2 taps or when a given ``scratch_bytes`` does not hold
    one batch entry: the composed plan takes those).  ``partials`` workgroups share a channel's
    sum (default: enough that channels * partials fills the device; capped by the (row, block) pairs of a channel); the
    order of every sum is fixed by the plan, so two runs give the same bits.  ``pregate`` / ``postgate`` = True make it the
    filter gradient of the gated forward plan ``y = b * conv(a * x)``: ``u`` = a * x and the gradient b * gy are formed in the
    kernel's two block loads (word 11 of the payload), one multiplication per sample, so the result has the bits of the ungated
    plan on the torch products ``a * x`` and ``b * gy`` (with ``io_dtype``: of the float32 plan on the float32 products of
    the widened tensors) without either product in memory; ``run`` / ``filter_grad`` of such a plan take ``pregate=`` of
    ``in_shape`` and / or ``postgate=`` of ``grad_shape`` with every exec.  A partitioned plan passes the gates on to its
    per-partition plans.  ``io_dtype`` = torch.bfloat16 or torch.float16 (with
    ``dtype`` = torch.float32 only): ``u`` and ``gy`` are tensors of it, widened exactly in the kernel's loads; the result
    stays float32 and equals the float32 plan's on the widened tensors bit for bit.  Every argument error is raised before
    any device work."""
    batch, channels, length, n, taps, offset, out_length, partition = _fftconv_plan_args(
        "plan_fftconv_grad", "filter-gradient", dtype, batch, channels, length, n, taps, offset, out_length, correlate, partition,
        io_dtype)
    if partials is not None:
        partials = int(partials)
        if partials < 1 or partials > 65535:
            raise MifftError(-5, f"plan_fftconv_grad: partials = {partials}: 1 .. 65535")
    if fused and partition is None:
        raise MifftError(-2, "plan_fftconv_grad: fused=True is the fused gradient of a PARTITIONED plan: it goes with taps=K, partition=Q")
    if scratch_bytes is not None and not fused:
        raise MifftError(-2, "plan_fftconv_grad: scratch_bytes bounds the spectra of the fused partitioned gradient (fused=True)")
    if fused:  # (the refusals first: lag groups and one entry's spectra, before any device work)
        g = _fftconv_fused_grad_geometry(n, length, out_length, taps, offset, correlate)
        if partials is not None:
            raise MifftError(ERR_UNSUPPORTED, "plan_fftconv_grad(fused=True): the partial sums of the lag-group stage are the "
                                              "library's choice (partials=None)")
        if g.Pg > _FUSED_GRAD_MAX_LAG_GROUPS:
            raise MifftError(ERR_UNSUPPORTED, f"plan_fftconv_grad(fused=True): taps = {taps} at n = {n} are {g.Pg} lag groups of "
                                              f"{g.H}, above {_FUSED_GRAD_MAX_LAG_GROUPS}; the composed per-partition plan "
                                              "(fused=False) has no such limit")
        if scratch_bytes is not None and int(scratch_bytes) < 1:
            raise MifftError(-5, f"plan_fftconv_grad: scratch_bytes = {scratch_bytes}: a positive number of bytes, or None")
        _fftconv_fused_grad_slabs(batch, _fftconv_fused_grad_entry_bytes(g, channels, dtype), scratch_bytes)
        return FusedPartConvGradPlan(dtype, batch, channels, length, n, offset, out_length, correlate,
                                     DeviceContext() if ctx is None else ctx, taps, partition, io_dtype=io_dtype, pregate=pregate,
                                     postgate=postgate, scratch_bytes=scratch_bytes)
    if partition is not None:  # (the composed gradient of a partitioned plan: PartConvGradPlan)
        return PartConvGradPlan(dtype, batch, channels, length, n, offset, out_length, correlate, DeviceContext() if ctx is None else ctx, taps,
                                partition, partials=partials, io_dtype=io_dtype, pregate=pregate, postgate=postgate)
    if partials is not None:  # (capped by the pairs of a channel)
        blocks = 1 if taps is None else _fftconv_ols_geometry(n, taps, offset, out_length, correlate)[3]
        partials = min(partials, batch * blocks)
    return ConvGradPlan(dtype, batch, channels, length, n, offset, out_length, correlate, DeviceContext() if ctx is None else ctx, taps=taps,
                        partials=partials, io_dtype=io_dtype, pregate=pregate, postgate=postgate)


def _fftconv_grad_plan(dtype, rows, D, L, n, taps, offset, out_length, correlate, device, Q=None, io_dtype=None, gates=0,
                       fused=False):
    """the cached filter-gradient plan of ``fftconv``'s forward plan of the same key (the caller holds _PLAN_CACHE_LOCK);
    ``fused``: the selector's answer (_fftconv_grad_fused), part of the key"""
    return _plan_cached(("fftconv_grad", dtype, rows, D, L, n, offset, out_length, bool(correlate)), device, lambda: plan_fftconv_grad(
        dtype, rows // D, D, L, n, taps=taps, offset=offset, out_length=out_length, partition=Q, correlate=correlate,
        ctx=DeviceContext(device), io_dtype=io_dtype, pregate=bool(gates & 1), postgate=bool(gates & 2), fused=bool(fused)),
        key_tail=(taps, Q, io_dtype, gates) + (("fused",) if fused else ()))  # (the composed plan's key is what it was)


def fftconv_filter_grad(x: "torch.Tensor", gy: "torch.Tensor", K: int, *, n: Optional[int] = None, mode: str = "causal",
                        correlate: bool = False, block: Optional[int] = None, partition=None, io_dtype=None,
                        pregate: Optional["torch.Tensor"] = None, postgate: Optional["torch.Tensor"] = None,
                        fused: Optional[bool] = None) -> "torch.Tensor":
    """The gradient of ``sum(gy * fftconv(x, k, n=n, mode=mode, correlate=correlate, block=block))`` with respect to a filter
    ``k`` of ``K`` taps, by the fused filter-gradient kernel in one launch (plus a sum of partials and one irfftn, both on
    ``channels`` rows): ``x`` (..., D, L) and ``gy`` of the result's shape (..., D, Lo) give (D, K); a 1-D ``x`` (L,) with
    ``gy`` (Lo,) gives (K,), the gradient of a 1-D filter.  (A 1-D filter shared by rows (..., L): reshape to (-1, 1, L) and take
    row 0.)  The choice of ``n`` / overlap-save mirrors ``fftconv``'s for the same arguments, so this is the gradient of THAT
    call, circular where it is.  With ``partition=`` (as ``fftconv``'s) it is the gradient of the partitioned call: one launch
    per partition (``fused=False``), or the fused plan that transforms every block once (``fused=True``:
    ``FusedPartConvGradPlan``); ``fused=None`` takes the fused plan where it was measured not slower (``_FFTCONV_FUSED_GRAD``)
    and the composed one everywhere else.  float32 / float64; other input is converted to float64.  Plans are cached like ``fftconv``'s.
    ``io_dtype`` = torch.bfloat16 or torch.float16: ``x`` and ``gy`` are read as tensors of it (no copy when they already
    are), widened exactly in the kernel's loads, and the result is float32 -- the bits of the float32 call on the widened
    tensors.  The partitioned route stays composed, one half-storage launch per partition.
    ``pregate`` / ``postgate``: the gradient of ``sum(gy * fftconv(x, k, pregate=a, postgate=b, ...))`` instead, the gates
    fused into the kernel's loads of ``x`` and ``gy`` (the bits of this call on ``a * x`` and ``b * gy``).  ``pregate`` has
    exactly ``x``'s shape, ``postgate`` exactly ``gy``'s (ValueError otherwise: nothing is broadcast); both are real, live on
    ``x``'s device and are converted as ``x`` is."""
    if x.is_complex() or gy.is_complex():
        raise MifftError(-3, "fftconv_filter_grad expects real tensors (complex rows are out of scope)")
    if mode not in _FFTCONV_MODES:
        raise ValueError(f"fftconv_filter_grad: mode must be one of {_FFTCONV_MODES}, got {mode!r}")
    if correlate and mode != "causal":
        raise ValueError(f"fftconv_filter_grad: correlate=True goes with mode='causal' only, got {mode!r}")
    if x.dim() < 1 or x.dim() != gy.dim():
        raise MifftError(-1, f"fftconv_filter_grad expects x (..., D, L) with gy (..., D, Lo), or x (L,) with gy (Lo,), got "
                             f"{tuple(x.shape)} and {tuple(gy.shape)}")
    logical = tuple(x.shape)
    L, K = int(logical[-1]), int(K)
    D = int(logical[-2]) if x.dim() >= 2 else 1
    if L < 2 or K < 1:
        raise MifftError(-2, f"fftconv_filter_grad: rows of {L} samples (at least 2) and filters of {K} taps (at least 1)")
    if io_dtype is not None and io_dtype not in _IO_DTYPES:
        raise MifftError(-4, f"fftconv_filter_grad: io_dtype is torch.bfloat16 or torch.float16 (or None), got {io_dtype}")
    dtype, sdt = _fftconv_dtypes(x, io_dtype)
    n, taps, Q = _fftconv_pick_part("fftconv_filter_grad", L, K, dtype, n, block, partition)
    offset, out_length = _fftconv_window(mode, L, K)
    use_fused = _fftconv_grad_fused(fused, sdt, n, K, Q)
    if tuple(gy.shape) != logical[:-1] + (out_length,):
        raise ValueError(f"fftconv_filter_grad: gy is {tuple(gy.shape)}, the result of that fftconv call is "
                         f"{logical[:-1] + (out_length,)}")
    for g, shape, what, of in ((pregate, logical, "pregate", "x"), (postgate, tuple(gy.shape), "postgate", "gy")):
        if g is None:
            continue
        if g.is_complex():
            raise MifftError(-3, f"fftconv_filter_grad: {what} must be real")
        if tuple(g.shape) != shape:
            raise ValueError(f"fftconv_filter_grad: {what} is {tuple(g.shape)}, {of} is {shape}: a gate has exactly that shape "
                             "(nothing is broadcast)")
        if g.device != x.device:
            raise MifftError(-10, f"fftconv_filter_grad: {what} lives on {g.device}, x on {x.device}")
    rows = math.prod(logical[:-1])
    if rows < 1:
        raise MifftError(-8, f"fftconv_filter_grad: no rows in {logical}")
    device = _signal_device(x, "x")
    if gy.device != x.device:
        raise MifftError(-10, f"fftconv_filter_grad: gy lives on {gy.device}, x on {x.device}")
    xr = x.detach().to(sdt).contiguous().reshape(rows, L, 1)
    gr = gy.detach().to(sdt).contiguous().reshape(rows, out_length, 1)
    a = None if pregate is None else pregate.detach().to(sdt).contiguous().reshape(rows, L, 1)
    b = None if postgate is None else postgate.detach().to(sdt).contiguous().reshape(rows, out_length, 1)
    gates = (1 if a is not None else 0) | (2 if b is not None else 0)
    with _PLAN_CACHE_LOCK:
        plan = _fftconv_grad_plan(dtype, rows, D, L, n, taps, offset, out_length, correlate, device, Q, io_dtype, gates, use_fused)
        gk = plan.filter_grad(xr, gr, K, pregate=a, postgate=b)
    return gk if x.dim() >= 2 else gk.reshape(K)


class _FFTConvFunction(torch.autograd.Function):
    """``fftconv`` with a backward (first order).  forward: the plain call, grad mode off.  backward, with u = a x,
    gv = b gy and G = rfft(k, n) + d: gu = the adjoint convolution of gv (one launch of the opposite-correlate plan),
    gx = a gu, ga = x gu, gb = gy v with v recomputed without the postgate, gk and gd from the fused filter gradient of
    (u, gv), both formed in its loads.  The filter spectra of the cached plans are rewritten from the saved k and skip by every launch here: a second
    layer of the same shape may have overwritten them since the forward.
    The seventh value of ``cfg`` is the selector's answer for a partitioned path (_fftconv_grad_fused, asked in the forward):
    the fused partitioned filter gradient, or the composed one.
    With ``io_dtype`` (the sixth value of ``cfg``) x, a, b, gy and every launch's result are tensors of it: gu comes from the
    half-storage plan (b fused into its load, a into its store when only x wants a gradient; modes with o > 0 pad gy and b
    separately instead of their product), the products of 16-bit tensors (a gu, x gu, gy v) are torch's, computed in float32
    and rounded once, and the filter gradient reads x and gy through the half-storage kernel.
    With gates the filter gradient is the gated filter-gradient plan on (x, gy, a, b) directly (``plan_fftconv_grad(pregate=,
    postgate=)``): the kernel forms a x and b gy in its loads -- on 16-bit rows as float32 products of the widened samples, so
    no product is rounded to 16 bits -- and neither product nor any float32 copy reaches memory.  The torch product
    gv = b gy is formed only for the gx route of a mode with o > 0 on float rows, which pads it."""

    @staticmethod
    def forward(ctx, x, k, pregate, postgate, skip_t, skip_f, cfg):
        n, taps, mode, correlate, Q, io, _ = cfg
        ctx.cfg, ctx.skip_f = cfg, skip_f
        ctx.save_for_backward(x, k, pregate, postgate, skip_t)
        return fftconv(x, k, mode=mode, correlate=correlate, pregate=pregate, postgate=postgate, io_dtype=io,
                       skip=skip_t if skip_t is not None else skip_f, **_fftconv_selector(n, taps, Q))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, k, a, b, skip_t = ctx.saved_tensors
        n, taps, mode, correlate, Q, io, fused = ctx.cfg
        skip = skip_t.detach() if skip_t is not None else ctx.skip_f
        need_x, need_k, need_a, need_b, need_d = ctx.needs_input_grad[:5]
        logical = tuple(x.shape)
        L, K = int(logical[-1]), int(k.shape[-1])
        D = int(k.shape[0]) if k.dim() == 2 else 1
        dtype, sdt = _fftconv_dtypes(x, io)
        o, Lo = _fftconv_window(mode, L, K)
        rows = math.prod(logical[:-1])
        device = x.device.index
        gyr = gy.to(sdt).contiguous().reshape(rows, Lo)  # (sum().backward() hands in an expanded tensor)
        xr = x.to(sdt).contiguous().reshape(rows, L)
        ar = None if a is None else a.to(sdt).contiguous().reshape(rows, L)
        br = None if b is None else b.to(sdt).contiguous().reshape(rows, Lo)
        gx = gk = ga = gb = gd = None
        gv = None
        if io is None and o > 0 and (need_x or need_a):  # (the one route that reads the product: it is padded below)
            gv = gyr if br is None else br * gyr
        if need_x or need_a:
            # gu: the adjoint of u -> crop(conv(u, k') , o, Lo), one launch of the existing kernels on the gradient put at o
            fuse_a = ar is not None and need_x and not need_a
            if o > 0 and io is None:
                src, pre = torch.nn.functional.pad(gv, (o, 0)), None
            elif o > 0:  # (16-bit rows: gy and b padded apart, multiplied in the kernel's load, so that no product is rounded)
                src, pre = torch.nn.functional.pad(gyr, (o, 0)), None if br is None else torch.nn.functional.pad(br, (o, 0))
            else:
                src, pre = gyr, br
            if src.shape[-1] < 2:
                src = torch.nn.functional.pad(src, (0, 1))
                pre = None if pre is None else torch.nn.functional.pad(pre, (0, 1))
            Lin = int(src.shape[-1])
            gates = (1 if pre is not None else 0) | (2 if fuse_a else 0)
            out = torch.empty((rows, L, 1), dtype=sdt, device=x.device)
            with _PLAN_CACHE_LOCK:
                plan = _fftconv_fwd_plan(dtype, rows, D, Lin, n, taps, 0, L, not correlate, device, gates, Q, io)
                _fftconv_exec(plan, out, src.reshape(rows, Lin, 1), k.detach(), skip,
                              None if pre is None else pre.reshape(rows, Lin, 1), ar.reshape(rows, L, 1) if fuse_a else None)
            gu = out.reshape(rows, L)
            if ar is None or fuse_a:
                gx = gu
            else:
                gx = ar * gu if need_x else None
                ga = xr * gu
            if not need_x:
                gx = None
        if need_b:  # gb = gy v, v = conv(u, k) + d u recomputed by one forward launch without the postgate
            v = fftconv(x.detach(), k.detach(), mode=mode, correlate=correlate, pregate=None if a is None else a.detach(),
                        skip=skip, io_dtype=io, **_fftconv_selector(n, taps, Q))
            gb = gyr * v.reshape(rows, Lo)
        if need_k or need_d:  # (the gates go to the kernel's loads: the sums are those of the products a x and b gy, bit for bit)
            gates = (1 if ar is not None else 0) | (2 if br is not None else 0)
            with _PLAN_CACHE_LOCK:
                gplan = _fftconv_grad_plan(dtype, rows, D, L, n, taps, o, Lo, correlate, device, Q, io, gates, fused)
                g = gplan.filter_grad(xr.reshape(rows, L, 1), gyr.reshape(rows, Lo, 1), K,
                                      pregate=None if ar is None else ar.reshape(rows, L, 1),
                                      postgate=None if br is None else br.reshape(rows, Lo, 1))
            if need_k:
                gk = g.reshape(k.shape).to(k.dtype)
            if need_d:
                gd = g[:, 0].to(skip_t.dtype)
        back = lambda g, t: None if g is None else g.reshape(t.shape).to(t.dtype)
        return back(gx, x), gk, back(ga, a) if need_a else None, back(gb, b) if need_b else None, gd, None, None


def _imdct_norm_gain(norm, n: int, who: str) -> float:
    """the factor on the windowed cosine sum of the synthesis: 2 / n, or sqrt(2 / n) for ``norm="ortho"``"""
    return 2.0 / n if _mdct_norm_scale(norm, n, who) == 1.0 else math.sqrt(2.0 / n)


def _check_imdct_layout(in_shape: tuple, out_shape: tuple, n: int) -> tuple:
    """Layouts of an IMDCT plan (MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan): x (batch, F, n, 1) real -> out (batch, T, 1) real
    with F >= 2 and 2 <= T <= (F - 1) n; returns the dims (T, F, 2n)."""
    if len(in_shape) != 4 or len(out_shape) != 3:
        raise MifftError(-1, f"IMDCT layouts are (batch, F, n, 1) -> (batch, T, 1), got {in_shape} -> {out_shape}")
    if in_shape[-1] != 1 or out_shape[-1] != 1:
        raise MifftError(-3, f"both sides of an IMDCT plan have 1 component, got {in_shape[-1]} and {out_shape[-1]}")
    if in_shape[0] != out_shape[0]:
        raise MifftError(-2, f"batch {in_shape[0]} of x against {out_shape[0]} of out")
    n = _mdct_n(n, "IMDCT")
    F, T = in_shape[1], out_shape[1]
    if in_shape[2] != n:
        raise MifftError(-2, f"frames of {n} coefficients, x is {in_shape}")
    if F < 2:
        raise MifftError(-2, f"an IMDCT needs at least 2 frames, got {F}")
    if not 2 <= T <= (F - 1) * n:
        raise MifftError(-2, f"{F} frames of {n} coefficients cover 2 .. {(F - 1) * n} samples, out is {out_shape}")
    return (T, F, 2 * n)


def plan_imdct(dtype, batch: int, frames: int, n: int, *, length: Optional[int] = None, window=None, norm=None,
               ctx: Optional[DeviceContext] = None, whole_batch: int = 0) -> Plan:
    """Plan of the inverse MDCT of ``batch`` entries of ``frames`` frames of ``n`` coefficients (no reference counterpart;
    MIFFT_MDCT_TAG on a MIFFT_FLAG_ISTFT plan in include/mifft.h): it inverts ``plan_mdct`` under the same ``window`` (None:
    the sine window; else 2n values, taken by value) and ``norm``.  ``length``: output samples per entry, 2 .. (frames - 1) n,
    the default.  ``in_shape`` (batch, frames, n, 1), ``out_shape`` (batch, length, 1), both of ``dtype`` (float32 / float64);
    runs through ``fft(out, X, plan=plan)``, ``first=`` / ``count=`` included: one kernel launch -- the DCT-IV of every frame,
    the unfold to 2n samples, the window and the overlap-add of the two half-frames that meet in every sample happen in the
    store of a DCT-IV tile -- no tensor of frames, no memset; an entry's result is bit-identical for any batch and slab.
    Every argument error is raised before any device work."""
    batch, frames = int(batch), int(frames)
    if dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"an IMDCT plan reads and writes float32 or float64, got {dtype}")
    n = _mdct_n(n, "IMDCT")
    gain = _imdct_norm_gain(norm, n, "plan_imdct")
    T = (frames - 1) * n if length is None else int(length)
    in_shape, out_shape = (batch, frames, n, 1), (batch, T, 1)
    _check_imdct_layout(in_shape, out_shape, n)
    if window is not None:
        window = _window_f64(window, 2 * n)
    if ctx is None:
        ctx = DeviceContext()
    return Plan(dtype, dtype, in_shape, out_shape, device=ctx.device, whole_batch=whole_batch, imdct=n, imdct_gain=gain,
                stft_window=window)


def _imdct_composed(X: "torch.Tensor", w: "torch.Tensor", ortho: bool, length: int) -> "torch.Tensor":
    """The IMDCT as one DCT-IV launch plus torch, X (..., F, n) of float32 / float64 -> (..., length): a gather with a
    precomputed index / sign table that unfolds the n values of a frame to its 2n samples, the product with the window
    ((2 / n) w, or w under ortho), two shifted adds of the half-frames into a (..., (F + 1) n) buffer and the slice
    [n, n + length).  What ``imdct`` ran before the fused plan existed; it serves what that plan refuses."""
    F, n, dt = int(X.shape[-2]), int(X.shape[-1]), X.dtype
    # v = DCT-IV(X) / 2 (ortho: the orthonormal DCT-IV itself), then y = (2 / n) w * unfold(v) (ortho: w * unfold(v))
    v = dct(X, type=4, norm="ortho" if ortho else None)
    idx, sign = _mdct_unfold_tables(n)
    gain = sign * w * (1.0 if ortho else 1.0 / n)  # (the 1 / 2 of v and the 2 / n of the synthesis in one table)
    y = v.index_select(-1, idx.to(v.device)) * gain.to(device=v.device, dtype=dt)
    out = torch.zeros(tuple(X.shape[:-2]) + ((F + 1) * n,), dtype=dt, device=v.device)
    lead = tuple(X.shape[:-2])
    out[..., :F * n] += y[..., :n].reshape(lead + (F * n,))
    out[..., n:] += y[..., n:].reshape(lead + (F * n,))
    return out[..., n:n + length].contiguous()


def imdct(X: "torch.Tensor", *, window=None, norm=None, length: Optional[int] = None) -> "torch.Tensor":
    """The inverse of ``mdct`` under the same ``window`` and ``norm``: X of shape (..., F, n) real -> (..., length),
    ``length`` defaulting to (F - 1) n; the leading dims fold into the batch.  A window with w[j] ** 2 + w[j + n] ** 2 = 1
    (the default sine window, KBD, Vorbis) reproduces the signal exactly (time-domain aliasing cancellation).
    One kernel launch (``plan_imdct``): the DCT-IV of every frame, its unfold to 2n samples, the product with (2 / n) w
    (sqrt(2 / n) w under ``norm="ortho"``) and the sum of the two half-frames that meet in every output sample happen in the
    store of a DCT-IV tile; no tensor of frames and no zeroed buffer exist.  Input that is not float32 / float64 is converted
    to float64 first.  Plans are cached per (shape, dtype, n, norm, length, device, stream) and the window's contents; loops
    should use ``plan_imdct``.  Only what the fused plan refuses -- ``length == 1``, or a tile and carry beyond the CU's LDS
    (no admissible n today) -- runs the earlier composition, one DCT-IV launch plus torch.
    Differentiable with respect to ``X`` (first order): when grad mode is on and ``X.requires_grad``, the result carries a
    ``grad_fn`` whose backward is ONE launch of the fused MDCT (``plan_mdct`` with this call's gain as its scale and the same
    window) on the incoming gradient; it yields the mdct_frames(length, n) <= F frames that see a stored sample, and the
    frames beyond them get an exact zero.  The adjoint plan is made in the forward, under the key ``mdct`` itself uses.  With
    several batch entries AND a ``length`` cropped below the last frames, the plan's rows are shorter than the gradient's, so
    that case costs one zero-padded copy of gy (to (F - 1) n samples per entry) before its one launch.  The
    two cases that run the earlier composition raise a MifftError in the forward of a call that wants a gradient; the forward
    alone works under ``torch.no_grad()``.  Otherwise the call is what it has always been: same plan, same bits, no
    ``grad_fn``.  The window is taken by value and gets no gradient; there is no double backward."""
    if X.is_complex():
        raise MifftError(-3, "imdct expects a real tensor")
    if X.dim() < 2:
        raise MifftError(-1, "imdct expects a tensor of rank 2 or more: (F, n) or (..., F, n)")
    F, n = int(X.shape[-2]), _mdct_n(X.shape[-1], "imdct")
    gain = _imdct_norm_gain(norm, n, "imdct")
    if F < 2:
        raise MifftError(-2, f"imdct: at least 2 frames, got {F}")
    length = (F - 1) * n if length is None else int(length)
    if not 1 <= length <= (F - 1) * n:
        raise MifftError(-2, f"imdct: {F} frames of {n} coefficients cover 1 .. {(F - 1) * n} samples, length is {length}")
    w = None if window is None else _window_f64(window, 2 * n)
    dt = X.dtype if X.dtype in _OUT_DTYPES else torch.float64
    device = _signal_device(X, "X")
    ortho = gain != 2.0 / n
    lead = tuple(X.shape[:-2])
    wants_grad = torch.is_grad_enabled() and isinstance(X, torch.Tensor) and X.requires_grad
    if length == 1 and wants_grad:
        raise MifftError(ERR_UNSUPPORTED, "imdct: no gradient with respect to X for length = 1, which the fused plan refuses; "
                                          "the forward alone works under torch.no_grad()")
    if wants_grad:  # (w: a fresh host table, kept by value; the LDS refusal of the fused plan is raised in the forward)
        return _IMDCTFunction.apply(X, (dt, n, gain, None if w is None else w.clone(), length, device))
    if length == 1:
        return _imdct_composed(X.to(dt), mdct_window(n) if w is None else w, ortho, length)
    batch = math.prod(lead)
    in_shape, out_shape = (batch, F, n, 1), (batch, length, 1)
    Xr = X.to(dt).contiguous().reshape(in_shape)
    with _PLAN_CACHE_LOCK:
        try:
            plan = _plan_cached(("imdct", dt, in_shape, length, gain), device, lambda: Plan(
                dt, dt, in_shape, out_shape, device=device, imdct=n, imdct_gain=gain, stft_window=w), w)
        except MifftError as e:
            if e.status != ERR_UNSUPPORTED or "LDS" not in str(e):
                raise
            return _imdct_composed(X.to(dt), mdct_window(n) if w is None else w, ortho, length)
        out = torch.empty(out_shape, dtype=dt, device=Xr.device)
        fft(out, Xr, DeviceContext(device), plan=plan)
    return out.reshape(lead + (length,))


def stft(x: "torch.Tensor", n_fft: int, hop_length: Optional[int] = None, win_length: Optional[int] = None, window=None,
         center: bool = True, pad_mode: str = "reflect", normalized: bool = False, onesided: bool = True, *,
         out_dtype=None) -> "torch.Tensor":
    """torch.stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided=True, return_complex=True)
    of a real ``x`` of shape (T,) or (..., T); the leading dims fold into the batch.  ``hop_length`` defaults to n_fft // 4,
    ``win_length`` to n_fft; a shorter window is zero-padded on both sides to n_fft, as torch does; ``window=None`` is
    rectangular; ``normalized=True`` multiplies by n_fft ** -0.5 (folded into the window table).  ``pad_mode`` is "reflect" or
    "constant"; anything else, and ``onesided=False``, is MifftError -15.  Input that is not of ``out_dtype`` (default: that of
    a float32 / float64 ``x``, else float64) is converted first.
    Returns complex (..., n_fft // 2 + 1, F), torch's layout -- as a TRANSPOSED VIEW (``stride(-2) == 1``) of the frames-major
    (..., F, n_fft // 2 + 1) tensor the kernel writes; call ``.contiguous()`` where the bins-major order is needed in memory.
    One kernel launch: no padded copy of ``x``, no unfold, no tensor of frames (MIFFT_FLAG_STFT in include/mifft.h).
    Plans are cached per (shape, dtype, n_fft, hop, centring, device, stream) AND the window's contents: every call hashes the
    window's float64 values, so a window changed in place never meets a stale plan.  For a CUDA ``window`` that is one small
    synchronising device-to-host copy per call: loops should make the plan once with ``plan_stft`` and call ``fft``.
    Differentiable with respect to ``x`` (first order): when grad mode is on and ``x.requires_grad``, the result carries a
    ``grad_fn`` whose backward is ONE launch of the fused adjoint overlap-add (``plan_stft_adjoint``) on the incoming gradient,
    made frames-major first (a no-op for a gradient laid out like the view returned here); the gradient comes back in ``x``'s
    shape and dtype.  The adjoint plan is made, and cached under a key of its own, in the forward: what it cannot do --
    ``hop_length > n_fft``, float64 frames beyond 10240 samples -- is a MifftError there, while the forward alone works on an
    ``x`` without requires_grad.  Otherwise the call is what it has always been: same plan, same bits, no ``grad_fn``.  The
    window is taken by value and gets no gradient; there is no double backward."""
    return _stft_run("stft", x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, out_dtype,
                     None, None)


def _stft_run(who: str, x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, out_dtype, power,
              fb, logv=None, post=None) -> "torch.Tensor":
    """stft and spectrogram: the plain call (_stft_run_plain), through autograd exactly when grad mode is on and ``x`` requires
    grad; otherwise the call is what it has always been"""
    args = (who, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, out_dtype, power, fb, logv, post)
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
        return (_STFTFunction if power is None else _SpectrogramFunction).apply(x, args)
    return _stft_run_plain(who, x, *args[1:])


def _stft_table(window, win_length: int, n_fft: int, normalized: bool):
    """the window table of an stft call as n_fft float64 host values (centred, zero-padded, times n_fft ** -0.5 when
    normalized), or None for the rectangular window of a whole frame"""
    if window is None and win_length >= n_fft and not normalized:
        return None
    wl = torch.ones(win_length, dtype=torch.float64) if window is None else _window_f64(window, win_length)
    left = (n_fft - win_length) // 2
    w = torch.zeros(n_fft, dtype=torch.float64)
    w[left:left + win_length] = wl
    if normalized:
        w *= float(n_fft) ** -0.5
    return w


class _StftCall(NamedTuple):
    """An stft / spectrogram call as its autograd Function keeps it between forward and backward: everything by value -- the
    window as the float64 table of the forward (None: rectangular), ``fb`` and ``post`` as their float64 host matrices -- so
    that a window or matrix changed in place afterwards cannot give the backward another transform than the forward's."""
    who: str
    out_dtype: object
    batch: int
    length: int
    n_fft: int
    hop: int
    center: bool
    pad_mode: str
    window: object
    power: object
    fb: object
    logv: object
    post: object
    device: int

    @property
    def frames(self) -> int:
        return stft_frames(self.length, self.n_fft, self.hop, self.center)

    def run(self, x, power, fb=None, logv=None, post=None):
        """the plain call on these values (the table is the whole window: win_length = n_fft, nothing left to normalize)"""
        return _stft_run_plain(self.who, x, self.n_fft, self.hop, self.n_fft, self.window, self.center, self.pad_mode, False, True,
                               self.out_dtype, power, fb, logv, post)


def _stft_call(x, args) -> _StftCall:
    """the arguments of a call that _stft_run_plain has accepted, by value"""
    who, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, out_dtype, power, fb, logv, post = args
    n_fft = int(n_fft)
    hop_length = n_fft // 4 if hop_length is None else int(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    T = int(x.shape[-1])
    fbm = None if fb is None else _fb_f64(fb, n_fft // 2 + 1).clone()
    postm = None if post is None else _post_f64(post, int(fbm.shape[1])).clone()
    return _StftCall(who, out_dtype, x.numel() // T, T, n_fft, hop_length, bool(center), pad_mode,
                     _stft_table(window, win_length, n_fft, normalized), power, fbm, logv, postm, x.device.index)


def _stft_adjoint_plan(call: _StftCall, multiplier) -> StftAdjointPlan:
    """The cached adjoint plan of an stft / spectrogram call, looked up or made under the cache's lock, which the caller
    holds until its launch is enqueued: a plan the cache evicts is closed.  The forward of the autograd Functions asks for it
    first, so that what the adjoint cannot do is raised there; the backward asks again, since the plan of the forward may have
    left the cache in between."""
    w, device = call.window, call.device
    mode = call.pad_mode if call.center else None
    def build():
        try:
            return plan_stft_adjoint(call.out_dtype, call.batch, call.length, call.n_fft, call.hop, window=w, center=mode,
                                     multiplier=multiplier, ctx=DeviceContext(device))
        except MifftError as e:
            raise MifftError(e.status, f"{call.who}: no gradient with respect to x for these arguments ({e}); the forward "
                                       f"alone works on an x without requires_grad (or under torch.no_grad())") from None

    with _PLAN_CACHE_LOCK:  # (the multiplier stands between the window's digest and the device: the head is the finished key's)
        return _plan_cached(("stft_adjoint", call.out_dtype, (call.batch, call.length), call.n_fft, call.hop, mode,
                             _table_digest(w), multiplier), device, build)


class _STFTFunction(torch.autograd.Function):
    """stft with the gradient with respect to x: one adjoint launch (StftAdjointPlan, mode 1).  First order."""

    @staticmethod
    def forward(ctx, x, args):
        X = _stft_run_plain(args[0], x, *args[1:])
        ctx.call = _stft_call(x, args)
        _stft_adjoint_plan(ctx.call, None)
        ctx.x_shape, ctx.x_dtype = tuple(x.shape), x.dtype
        return X

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gX):
        call = ctx.call
        ctype = torch.complex64 if call.out_dtype == torch.float32 else torch.complex128
        # frames-major memory: a no-op for a gradient laid out like the view stft returns
        g = torch.view_as_real(gX.to(ctype).transpose(-1, -2).contiguous())
        with _PLAN_CACHE_LOCK:
            plan = _stft_adjoint_plan(call, None)
            gx = plan.apply(g.reshape(plan.in_shape))
        return gx.reshape(ctx.x_shape).to(ctx.x_dtype), None


class _SpectrogramFunction(torch.autograd.Function):
    """spectrogram (and so mfcc) with the gradient with respect to x.  Without fb / log / post: one stft launch recomputes X,
    one adjoint launch (mode 2 or 3) takes the incoming gradient as its factor.  With them the chain down to the bins is torch
    on band-sized tensors.  First order; the window, the filterbank and ``post`` get no gradient."""

    @staticmethod
    def forward(ctx, x, args):
        y = _stft_run_plain(args[0], x, *args[1:])
        ctx.call = _stft_call(x, args)
        _stft_adjoint_plan(ctx.call, int(ctx.call.power))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        call = ctx.call
        dt, dev = call.out_dtype, gy.device
        g = gy.to(dt).transpose(-1, -2)  # frames-major (..., F, width)
        if call.post is not None:  # gBands = gy @ post.T
            g = g @ call.post.to(device=dev, dtype=dt).transpose(0, 1)
        if call.logv is not None:  # y = a log2(max(v + add, amin)) + c: a / (ln 2 (v + add)) where v + add > amin, 0 elsewhere
            add, amin, a, _ = call.logv
            v = call.run(x, call.power, call.fb).transpose(-1, -2)
            s = v + add
            g = torch.where(s > amin, g * (a / math.log(2.0)) / s, torch.zeros_like(g))
        if call.fb is not None:  # gP = gBands @ fb.T
            g = g @ call.fb.to(device=dev, dtype=dt).transpose(0, 1)
        m = g.contiguous()
        Xf = torch.view_as_real(call.run(x, None).transpose(-1, -2).contiguous())
        with _PLAN_CACHE_LOCK:  # (the recomputing calls above may have pushed the forward's adjoint plan out of the cache)
            plan = _stft_adjoint_plan(call, int(call.power))
            gx = plan.apply(Xf.reshape(plan.in_shape), m.reshape(plan.mult_shape))
        return gx.reshape(tuple(x.shape)).to(x.dtype), None


def _stft_run_plain(who: str, x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, out_dtype, power,
                    fb, logv=None, post=None) -> "torch.Tensor":
    """stft (``power`` None) and spectrogram (``power`` 1 or 2, ``fb`` None or a (n_fft // 2 + 1, M) float64 host matrix,
    ``logv`` None or (add, amin, a, c), ``post`` None or an (M, Q) matrix)"""
    if not onesided:
        raise MifftError(ERR_UNSUPPORTED, f"{who}: onesided=False is not supported")
    if pad_mode not in ("reflect", "constant"):
        raise MifftError(ERR_UNSUPPORTED, f"{who}: pad_mode must be \"reflect\" or \"constant\", got {pad_mode!r}")
    if x.is_complex():
        raise MifftError(-3, f"{who} expects a real tensor")
    if x.dim() < 1:
        raise MifftError(-1, f"{who} expects a tensor of rank 1 or more: (T,) or (..., T)")
    n_fft = int(n_fft)
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"{who} with an odd n_fft or one below 8 ({n_fft}) is not supported")
    hop_length = n_fft // 4 if hop_length is None else int(hop_length)
    FLAG_STFT_HOP(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    if not 0 < win_length <= n_fft:
        raise MifftError(-2, f"{who}: 0 < win_length <= n_fft, got win_length = {win_length}, n_fft = {n_fft}")
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.float64
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"{who}: out_dtype must be float32 or float64, got {out_dtype}")
    mode = (pad_mode if center else None)
    logical = tuple(x.shape)
    T, batch = logical[-1], math.prod(logical[:-1])
    frames = stft_frames(T, n_fft, hop_length, bool(center))
    bins = n_fft // 2 + 1
    if fb is not None:
        fb = _fb_f64(fb, bins)
    width = bins if fb is None else int(fb.shape[1])
    if post is not None:
        post = _post_f64(post, None if fb is None else width)
        width = int(post.shape[1])
    in_shape, out_shape = (batch, T, 1), (batch, frames, width, 2 if power is None else 1)
    _check_stft_layout(in_shape, (batch, frames, bins, 2), hop_length, mode)
    w = _stft_table(window, win_length, n_fft, normalized)
    device = _signal_device(x, "x")
    xr = x.to(out_dtype).contiguous().reshape(in_shape)
    out = torch.empty(out_shape, dtype=out_dtype, device=xr.device)
    tail = ()
    if power is not None:  # (the stft key as it has always been, then what the spectrogram adds)
        tail += (power, None if fb is None else (tuple(fb.shape), _table_digest(fb)))
    if logv is not None or post is not None:  # (and what the log stage and the matrix after the bands add)
        tail += (logv, None if post is None else (tuple(post.shape), _table_digest(post)))
    with _PLAN_CACHE_LOCK:
        plan = _plan_cached(("stft", out_dtype, in_shape, n_fft, hop_length, mode), device, lambda: Plan(
            out_dtype, out_dtype, in_shape, out_shape, device=device, stft_hop=hop_length, stft_center=mode, stft_window=w,
            stft_power=power, stft_fb=fb, stft_log=logv, stft_post=post), w, key_tail=tail)
        fft(out, xr, DeviceContext(device), plan=plan)
    if power is not None:
        return out.reshape(logical[:-1] + (frames, width)).transpose(-1, -2)
    return torch.view_as_complex(out).reshape(logical[:-1] + (frames, n_fft // 2 + 1)).transpose(-1, -2)


def spectrogram(x: "torch.Tensor", n_fft: int, hop_length: Optional[int] = None, win_length: Optional[int] = None,
                window=None, center: bool = True, pad_mode: str = "reflect", normalized: bool = False, power=2.0, *,
                fb=None, out_dtype=None, onesided: bool = True, log=None, amin: float = 1e-10, eps: float = 0.0,
                ref: float = 1.0, post=None) -> "torch.Tensor":
    """torch.stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided=True,
    return_complex=True).abs().pow(power) of a real ``x`` of shape (T,) or (..., T), ``power`` 1 (magnitude) or 2 (power), in one
    kernel launch that never writes the complex spectrogram; every argument it shares with ``stft`` means what it means
    there.  ``normalized=True`` is torch.stft's, a factor n_fft ** -0.5 on X -- not torchaudio's window normalisation.
    ``fb``: a filterbank of shape (n_fft // 2 + 1, M), any real tensor or array on any device, taken by value as float64 like
    the window; the result is then (fb.T @ .) along the frequency dim, M bands per frame.  That is the orientation of
    torchaudio.functional.melscale_fbanks; a librosa-style (M, n_fft // 2 + 1) matrix must be transposed by the caller.  The
    bands are summed over the span of each column's non-zero rows: a dense matrix is correct but slow.  ``melscale_fbanks``
    makes a mel filterbank.
    ``log`` / ``amin`` / ``eps`` / ``ref``: a log stage in the same launch, as in ``plan_spectrogram`` -- "log":
    ln(max(v + eps, amin)); "log10": base 10; "db": torchaudio's amplitude_to_DB(v, multiplier 10 for ``power=2`` / 20 for
    ``power=1``, amin, db_multiplier=log10(max(amin, ref))) without top_db.  ``ref`` with any other ``log`` is -15.  There is
    no ``top_db`` and no Whisper ``max - 8`` clamp, which need the maximum over a whole entry; on the small output that is one
    line, ``y = torch.maximum(y, y.amax(dim=(-2, -1), keepdim=True) - 80.0)`` (Whisper: ``- 8.0`` on log10).
    ``post``: an (M, Q) real matrix after the bands (and the log stage), taken by value as float64; needs ``fb`` and
    M <= n_fft // 2 - 1; the result has Q values per frame.  With ``create_dct`` that is the MFCC (``mfcc``).
    Returns real (..., n_fft // 2 + 1 or M or Q, F) as a TRANSPOSED VIEW (``stride(-2) == 1``) of the frames-major tensor the kernel
    writes, exactly as ``stft`` does.  ``power`` other than 1 or 2 is MifftError -15; so is ``power=None``: the complex
    spectrogram is ``stft``.  A filterbank of another shape is -2.  Plans are cached as those of ``stft``, the key extended by
    the power and a digest of the filterbank's values (and of ``post``, and the log stage), so a matrix changed in place never
    meets a stale plan; loops should make the plan once with ``plan_spectrogram`` and call ``fft``.
    Differentiable with respect to ``x`` (first order), exactly when grad mode is on and ``x.requires_grad``; otherwise the
    call is what it has always been.  Without ``fb`` / ``log`` / ``post`` the backward is two launches and no torch op on a
    spectrogram-sized tensor: one ``stft`` launch recomputes X, one adjoint launch (``plan_stft_adjoint(multiplier=power)``) takes
    the incoming gradient m as a per-bin factor in its load -- 2 m X, or m X / abs(X) with zero where abs(X) is, torch's
    ``abs`` backward -- so that the product never exists in memory.  With them the chain down to the bins is torch on
    band-sized tensors first: ``gy @ post.T``, the log stage's derivative (zero where the clamp at ``amin`` holds; its argument
    recomputed by one forward launch without ``log`` / ``post``), ``@ fb.T``.  The adjoint plan is made in the forward, as in
    ``stft``, with the same refusals.  The window, ``fb`` and ``post`` are taken by value and get no gradient."""
    if power is None:
        raise MifftError(ERR_UNSUPPORTED, "spectrogram: power=None is the complex spectrogram: use stft")
    power = _spec_power(power)
    logv = _log_stage(log, amin, eps, ref, power)
    if post is not None and fb is None:
        _post_f64(post, None)
    return _stft_run("spectrogram", x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided,
                     out_dtype, power, fb, logv, post)


def _mel(f, scale: str):
    import numpy as np
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f >= 1000.0, 15.0 + 27.0 * np.log(np.maximum(f, 1000.0) / 1000.0) / np.log(6.4), 3.0 * f / 200.0)


def _mel_to_hz(m, scale: str):
    import numpy as np
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) * (np.maximum(m, 15.0) - 15.0) / 27.0), 200.0 * m / 3.0)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, norm=None,
                    mel_scale: str = "htk") -> "torch.Tensor":
    """The triangular mel filterbank of torchaudio.functional.melscale_fbanks as a float64 (n_freqs, n_mels) host tensor, the
    orientation ``fb=`` takes.  Pure host arithmetic, by this definition and no other:
        all_freqs = linspace(0, sample_rate // 2, n_freqs); m_pts = linspace(mel(f_min), mel(f_max), n_mels + 2); f_pts = hz(m_pts)
        fb[k, m] = max(0, min((all_freqs[k] - f_pts[m]) / (f_pts[m+1] - f_pts[m]),
                              (f_pts[m+2] - all_freqs[k]) / (f_pts[m+2] - f_pts[m+1])))
    ``norm="slaney"`` multiplies column m by 2 / (f_pts[m+2] - f_pts[m]).  ``mel_scale`` "htk": mel(f) = 2595 log10(1 + f / 700);
    "slaney": 3 f / 200 below 1000 Hz and 15 + 27 ln(f / 1000) / ln 6.4 from there; hz() is the inverse of each.
    Argument errors are MifftError."""
    import numpy as np
    if norm is not None and norm != "slaney":
        raise MifftError(ERR_UNSUPPORTED, f"norm must be None or \"slaney\", got {norm!r}")
    if mel_scale not in ("htk", "slaney"):
        raise MifftError(ERR_UNSUPPORTED, f"mel_scale must be \"htk\" or \"slaney\", got {mel_scale!r}")
    n_freqs, n_mels, sample_rate = int(n_freqs), int(n_mels), int(sample_rate)
    f_min, f_max = float(f_min), float(f_max)
    if n_freqs < 2 or n_mels < 1 or sample_rate < 2:
        raise MifftError(-2, f"n_freqs >= 2, n_mels >= 1 and sample_rate >= 2, got {n_freqs}, {n_mels}, {sample_rate}")
    if not 0.0 <= f_min < f_max or f_max == float("inf"):
        raise MifftError(-2, f"0 <= f_min < f_max, both finite, got {f_min}, {f_max}")
    all_freqs = np.linspace(0.0, float(sample_rate // 2), n_freqs)
    f_pts = _mel_to_hz(np.linspace(float(_mel(f_min, mel_scale)), float(_mel(f_max, mel_scale)), n_mels + 2), mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]                       # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:] - f_pts[:-2]))[None, :]
    return torch.from_numpy(np.ascontiguousarray(fb))


def create_dct(n_mfcc: int, n_mels: int, norm="ortho") -> "torch.Tensor":
    """The DCT-II matrix of torchaudio.functional.create_dct as a float64 (n_mels, n_mfcc) host tensor, the orientation
    ``post=`` takes: D[m, q] = cos(pi / n_mels * (m + 0.5) * q), times 2 for ``norm=None``; for "ortho" column 0 times
    1 / sqrt(2), then everything times sqrt(2 / n_mels).  ``y @ create_dct(Q, M, norm)`` is scipy.fft.dct(y, type=2,
    norm=norm)[..., :Q]."""
    import numpy as np
    if norm is not None and norm != "ortho":
        raise MifftError(ERR_UNSUPPORTED, f"norm must be None or \"ortho\", got {norm!r}")
    n_mfcc, n_mels = int(n_mfcc), int(n_mels)
    if n_mels < 1 or n_mfcc < 1:
        raise MifftError(-2, f"n_mfcc >= 1 and n_mels >= 1, got {n_mfcc}, {n_mels}")
    d = np.cos(np.pi / n_mels * (np.arange(n_mels, dtype=np.float64)[:, None] + 0.5) * np.arange(n_mfcc, dtype=np.float64)[None, :])
    if norm is None:
        d *= 2.0
    else:
        d[:, 0] *= 1.0 / np.sqrt(2.0)
        d *= np.sqrt(2.0 / n_mels)
    return torch.from_numpy(d)


def mfcc(x: "torch.Tensor", sample_rate: int, n_mfcc: int = 40, *, n_fft: int = 400, hop_length: Optional[int] = None,
         win_length: Optional[int] = None, window=None, n_mels: int = 128, f_min: float = 0.0, f_max: Optional[float] = None,
         mel_norm=None, mel_scale: str = "htk", dct_norm="ortho", log="db", amin: float = 1e-10, eps: float = 0.0,
         center: bool = True, pad_mode: str = "reflect") -> "torch.Tensor":
    """Mel-frequency cepstral coefficients of a real ``x`` of shape (T,) or (..., T) in one kernel launch:
    ``spectrogram(x, n_fft, ..., power=2, fb=melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate, mel_norm,
    mel_scale), log=log, amin=amin, eps=eps, post=create_dct(n_mfcc, n_mels, dct_norm))``; ``f_max`` defaults to
    sample_rate // 2, ``hop_length`` to n_fft // 4, ``window=None`` is rectangular (torchaudio's MFCC uses a Hann window: pass
    one).  ``log=None`` skips the log stage.  torchaudio's and librosa's default ``top_db=80`` clamp is NOT applied: it needs
    the maximum over a whole entry, which one pass over the frames does not have.  Needs n_mels <= n_fft // 2 - 1.
    Returns (..., n_mfcc, F) as the same transposed view as ``spectrogram``.  Every argument error is a MifftError before any
    device work.  Differentiable with respect to ``x`` as ``spectrogram`` is (the DCT matrix, the log stage and the filterbank
    in torch on band-sized tensors, then the fused adjoint); the filterbank and the DCT matrix get no gradient."""
    n_fft = int(n_fft)
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"mfcc with an odd n_fft or one below 8 ({n_fft}) is not supported")
    if int(n_mfcc) > int(n_mels):
        raise MifftError(-2, f"n_mfcc ({n_mfcc}) cannot exceed n_mels ({n_mels})")
    fb = melscale_fbanks(n_fft // 2 + 1, f_min, float(int(sample_rate) // 2) if f_max is None else f_max, n_mels, sample_rate,
                         mel_norm, mel_scale)
    if int(n_mels) > n_fft // 2 - 1:
        raise MifftError(ERR_UNSUPPORTED, f"mfcc needs n_mels <= n_fft // 2 - 1 = {n_fft // 2 - 1}, got {n_mels}")
    return spectrogram(x, n_fft, hop_length, win_length, window, center, pad_mode, False, 2.0, fb=fb, log=log, amin=amin,
                       eps=eps, post=create_dct(n_mfcc, n_mels, dct_norm))


def istft(X: "torch.Tensor", n_fft: int, hop_length: Optional[int] = None, win_length: Optional[int] = None, window=None,
          center: bool = True, normalized: bool = False, onesided: Optional[bool] = None, length: Optional[int] = None,
          return_complex: bool = False, *, out_dtype=None) -> "torch.Tensor":
    """torch.istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided=True, length, return_complex=False)
    of a complex ``X`` of shape (n_fft // 2 + 1, F) or (..., n_fft // 2 + 1, F), torch's layout; the leading dims fold into
    the batch.  ``hop_length`` defaults to n_fft // 4, ``win_length`` to n_fft; a shorter window is zero-padded on both sides
    to n_fft, as torch does; ``window=None`` is rectangular.  Returns real (..., length), ``length`` defaulting to
    istft_length(F, n_fft, hop_length, center).  ``onesided=False``, ``return_complex=True``, an odd n_fft and a ``length``
    beyond what the frames cover (torch zero-pads) are MifftError -15; so is a window whose squared overlap-add vanishes in
    the output range (torch raises for it too).  Input that is not of ``out_dtype``'s complex type (default: that of a
    complex64 / complex128 ``X``) is converted first.
    The kernel reads frames-major (..., F, n_fft // 2 + 1) memory: when ``X.transpose(-1, -2)`` is contiguous -- exactly the
    view ``stft`` returns -- X is used as it lies, with no copy; otherwise ONE transposing copy is made first.
    One kernel launch: no tensor of frames, no fold, no memset (MIFFT_FLAG_ISTFT in include/mifft.h).  Plans are cached like
    ``stft``'s: per (shape, dtype, n_fft, hop, centring, length, gain, device, stream) AND the window's contents.
    Differentiable with respect to ``X`` (first order): when grad mode is on and ``X.requires_grad``, the result carries a
    ``grad_fn`` whose backward is ONE launch of the fused adjoint (``plan_istft_adjoint``) on the incoming gradient: the STFT
    tile with the reciprocal envelope in its load.  The gradient comes back in ``X``'s shape and dtype, as the transposed view
    of the frames-major tensor the kernel writes (no transposing copy), in torch's convention dL/dRe X + i dL/dIm X; the
    imaginary parts of bins 0 and n_fft // 2, which the forward ignores, get an exact zero.  The adjoint plan is made, and
    cached under a key of its own, in the forward, so that what it refuses is a MifftError there.  Otherwise the call is what
    it has always been: same plan, same bits, no ``grad_fn``.  The window is taken by value and gets no gradient; there is no
    double backward."""
    call = _istft_call(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex, out_dtype)
    if torch.is_grad_enabled() and isinstance(X, torch.Tensor) and X.requires_grad:
        return _ISTFTFunction.apply(X, call)
    return _istft_exec(call, X)


class _IstftCall(NamedTuple):
    """An istft call that has passed its checks, by value (the window as the float64 table of the forward; None:
    rectangular), as the plain call runs it and as its autograd Function keeps it between forward and backward"""
    out_dtype: object
    lead: tuple
    batch: int
    frames: int
    n_fft: int
    hop: int
    center: bool
    length: int
    gain: float
    window: object
    device: int

    @property
    def in_shape(self) -> tuple:
        return (self.batch, self.frames, self.n_fft // 2 + 1, 2)

    @property
    def out_shape(self) -> tuple:
        return (self.batch, self.length, 1)


def _istft_call(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex,
                out_dtype) -> _IstftCall:
    """the checks of ``istft``, in the order they have always run, and the call by value"""
    if onesided is not None and not onesided:
        raise MifftError(ERR_UNSUPPORTED, "istft: onesided=False is not supported")
    if return_complex:
        raise MifftError(ERR_UNSUPPORTED, "istft: return_complex=True is not supported")
    if not X.is_complex():
        raise MifftError(-3, "istft expects a complex tensor")
    if X.dim() < 2:
        raise MifftError(-1, "istft expects a tensor of rank 2 or more: (n_fft // 2 + 1, F) or (..., n_fft // 2 + 1, F)")
    n_fft = int(n_fft)
    if n_fft % 2 or n_fft < 8:
        raise MifftError(ERR_UNSUPPORTED, f"istft with an odd n_fft or one below 8 ({n_fft}) is not supported")
    if X.shape[-2] != n_fft // 2 + 1:
        raise MifftError(-2, f"istft: X has {X.shape[-2]} bins, n_fft = {n_fft} needs {n_fft // 2 + 1}")
    hop_length = n_fft // 4 if hop_length is None else int(hop_length)
    FLAG_STFT_HOP(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    if not 0 < win_length <= n_fft:
        raise MifftError(-2, f"istft: 0 < win_length <= n_fft, got win_length = {win_length}, n_fft = {n_fft}")
    if out_dtype is None:
        out_dtype = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(X.dtype, torch.float64)
    if out_dtype not in _OUT_DTYPES:
        raise MifftError(-4, f"istft: out_dtype must be float32 or float64, got {out_dtype}")
    logical = tuple(X.shape)
    frames, batch = logical[-1], math.prod(logical[:-2])
    covered = istft_length(frames, n_fft, hop_length, False) - (n_fft // 2 if center else 0)
    T = istft_length(frames, n_fft, hop_length, bool(center)) if length is None else int(length)
    if T > covered:
        raise MifftError(ERR_UNSUPPORTED, f"istft: length = {T} beyond the {covered} samples the frames cover (zero-padding "
                                          f"is not supported)")
    in_shape, out_shape = (batch, frames, n_fft // 2 + 1, 2), (batch, T, 1)
    _check_istft_layout(in_shape, out_shape, hop_length, bool(center))
    w = None
    if window is not None or win_length < n_fft:
        wl = torch.ones(win_length, dtype=torch.float64) if window is None else _window_f64(window, win_length)
        left = (n_fft - win_length) // 2
        w = torch.zeros(n_fft, dtype=torch.float64)
        w[left:left + win_length] = wl
    gain = float(n_fft) ** 0.5 if normalized else 1.0
    device = _signal_device(X, "X")
    return _IstftCall(out_dtype, logical[:-2], batch, frames, n_fft, hop_length, bool(center), T, gain, w, device)


def _istft_exec(call: _IstftCall, X: "torch.Tensor") -> "torch.Tensor":
    """the one launch of an accepted istft call"""
    out_dtype, in_shape, out_shape, device, w = call.out_dtype, call.in_shape, call.out_shape, call.device, call.window
    ctype = torch.complex64 if out_dtype == torch.float32 else torch.complex128
    # frames-major memory: a no-op for the view stft returns, one transposing copy otherwise
    xf = X.to(ctype).transpose(-1, -2).contiguous()
    xr = torch.view_as_real(xf).reshape(in_shape)
    out = torch.empty(out_shape, dtype=out_dtype, device=xr.device)
    with _PLAN_CACHE_LOCK:
        plan = _plan_cached(("istft", out_dtype, in_shape, call.n_fft, call.hop, call.center, call.length, call.gain), device,
                            lambda: Plan(out_dtype, out_dtype, in_shape, out_shape, device=device, istft_hop=call.hop,
                                         stft_center=call.center, stft_window=w, istft_gain=call.gain), w)
        fft(out, xr, DeviceContext(device), plan=plan)
    return out.reshape(call.lead + (call.length,))


def _istft_adjoint_plan(call: _IstftCall) -> Plan:
    """The cached adjoint plan of an istft call, looked up or made under the cache's lock, which the caller holds until its
    launch is enqueued.  The forward of _ISTFTFunction asks for it first, so that a refusal is raised there; the backward asks
    again, since the plan may have left the cache in between."""
    w, device = call.window, call.device
    def build():
        try:
            return plan_istft_adjoint(call.out_dtype, call.batch, call.frames, call.n_fft, call.hop, window=w, center=call.center,
                                      gain=call.gain, length=call.length, ctx=DeviceContext(device))
        except MifftError as e:
            raise MifftError(e.status, f"istft: no gradient with respect to X for these arguments ({e}); the forward alone "
                                       f"works on an X without requires_grad (or under torch.no_grad())") from None

    with _PLAN_CACHE_LOCK:
        return _plan_cached(("istft_adjoint", call.out_dtype, call.in_shape, call.n_fft, call.hop, call.center, call.length,
                             call.gain), device, build, w)


class _ISTFTFunction(torch.autograd.Function):
    """istft with the gradient with respect to X: one launch of the STFT tile with the envelope in its load
    (plan_istft_adjoint).  First order."""

    @staticmethod
    def forward(ctx, X, call):
        y = _istft_exec(call, X)
        _istft_adjoint_plan(call)
        ctx.call, ctx.x_dtype = call, X.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        call = ctx.call
        g = gy.to(call.out_dtype).contiguous().reshape(call.out_shape)
        out = torch.empty(call.in_shape, dtype=call.out_dtype, device=g.device)
        with _PLAN_CACHE_LOCK:
            fft(out, g, DeviceContext(call.device), plan=_istft_adjoint_plan(call))
        # bins-major, X's layout, as the transposed view of the frames-major tensor the kernel wrote
        gX = torch.view_as_complex(out).reshape(call.lead + (call.frames, call.n_fft // 2 + 1)).transpose(-1, -2)
        return gX.to(ctx.x_dtype), None
