"""What the inverse-STFT gradient tests share: the shapes, the windows, the reference -- torch.autograd over torch.istft on the
CPU in fp64, on inputs rounded to the dtype under test -- and an fp64 numpy model of the adjoint exactly as the kernel computes
it (the reciprocal envelope with zeros where the envelope vanishes, zeros selected outside [0, T), the analysis table
2 g w / n, the halved bins 0 and n / 2 with exact-zero imaginary parts), which tests/test_istft_grad_host.py holds against the
reference."""
import functools

import numpy as np
import torch

# (B, F, n_fft, hop, centred, window, win_length, length, normalized): the smallest at which each mechanism can go wrong
SMALL_SHAPES = [
    (3, 13, 16, 4, True, "hann", 16, None, False),
    (3, 11, 16, 5, True, None, 16, None, False),      # odd hop, rectangular: unaligned pairs
    (3, 12, 16, 3, False, "hamming", 16, None, False),  # uncentred
    (2, 4, 16, 16, True, None, 16, None, False),      # hop = n: no overlap
    (2, 9, 32, 7, True, "hann", 32, 38, False),       # cropped: the last frame of each entry is an exact zero
    (2, 7, 16, 5, True, "hann", 12, 20, False),       # short window, envelope 0 below the stored range: the last two frames zero
    (2, 9, 16, 4, True, "hann", 16, None, True),      # normalized
    (2, 6, 16, 4, False, "hamming", 16, 30, True),    # uncentred, cropped
]
WALK = (5, 150, 16, 3, True, "hamming", 16, None, False)      # several tiles per entry, tiles that wrap into the next entry
MID = (2, 36, 1024, 256, True, "hann", 1024, None, False)
BIG = (1, 7, 16384, 4096, True, "hann", 16384, None, False)   # fp32 only
# the frames of a shape (by its index in SMALL_SHAPES) that see no stored sample: an exact zero
ZERO_FRAMES = {4: [8], 5: [5, 6]}


def window_of(name, n):
    """periodic windows, as torch.hann_window / torch.hamming_window; None: rectangular"""
    if name is None:
        return None
    a = {"hann": 0.5, "hamming": 0.54}[name]
    return a - (1.0 - a) * np.cos(2.0 * np.pi * np.arange(n) / n)


def table_of(name, win_length, n):
    """the window of a shape zero-padded to n on both sides, as torch pads it (float64), or None for a whole rectangular frame"""
    if name is None and win_length >= n:
        return None
    w = np.zeros(n)
    left = (n - win_length) // 2
    w[left:left + win_length] = 1.0 if name is None else window_of(name, win_length)
    return w


def length_of(shape):
    _, F, n, hop, centred, _, _, length, _ = shape
    return n + hop * (F - 1) - (2 * (n // 2) if centred else 0) if length is None else length


def inputs(shape, dtype, seed=0):
    """(X complex (B, bins, F), gy (B, T)) as float64 / complex128 numpy arrays whose values are those of ``dtype`` (np.float32
    or np.float64)"""
    B, F, n = shape[:3]
    rng = np.random.default_rng(1000 + seed)
    X = (rng.standard_normal((B, n // 2 + 1, F)) + 1j * rng.standard_normal((B, n // 2 + 1, F)))
    gy = rng.standard_normal((B, length_of(shape)))
    if dtype == np.float32:
        X = X.astype(np.complex64).astype(np.complex128)
        gy = gy.astype(np.float32).astype(np.float64)
    return X, gy


def torch_istft(X, shape):
    """torch.istft of a (B, bins, F) complex tensor under the arguments of ``shape``"""
    _, _, n, hop, centred, wname, wl, length, normalized = shape
    w = torch.as_tensor(np.ones(wl) if wname is None else window_of(wname, wl), dtype=X.real.dtype, device=X.device)
    return torch.istft(X, n, hop, wl, window=w, center=centred, normalized=normalized, length=length)


def reference(shape, dtype, seed=0):
    """(X, gy, gX): gX = the gradient of <torch.istft(X), gy> with respect to X, complex128 (B, bins, F)"""
    return _reference(shape, np.dtype(dtype).name, seed)


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype_name, seed):
    X, gy = inputs(shape, np.dtype(dtype_name).type, seed)
    Xt = torch.from_numpy(X).requires_grad_(True)
    torch_istft(Xt, shape).backward(torch.from_numpy(gy))
    return X, gy, Xt.grad.numpy()


def envelope(w, n, hop, F):
    """E[u] = sum_f w[u - f hop] ** 2 at every padded sample u < n + hop (F - 1)"""
    w = np.ones(n) if w is None else w
    E = np.zeros(n + hop * (F - 1))
    for f in range(F):
        E[f * hop:f * hop + n] += w * w
    return E


def adjoint_model(gy, shape):
    """The adjoint as the kernel computes it, in float64: gy (B, T) -> complex (B, F, n / 2 + 1), frames-major."""
    _, F, n, hop, centred, wname, wl, _, normalized = shape
    gy = np.asarray(gy, dtype=np.float64)
    B, T = gy.shape
    N, c = n // 2, (n // 2 if centred else 0)
    w = table_of(wname, wl, n)
    w = np.ones(n) if w is None else w
    g = float(np.float32(np.sqrt(float(n)))) if normalized else 1.0  # (the gain travels as the forward's does: float32's)
    E = envelope(w, n, hop, F)
    inv = np.where(E != 0.0, 1.0 / np.where(E != 0.0, E, 1.0), 0.0)
    L = n + hop * (F - 1)
    assert T <= L - c
    gyp = np.zeros((B, L))          # zeros selected outside [c, c + T)
    gyp[:, c:c + T] = gy * inv[c:c + T]
    wa = 2.0 * g * w / n
    out = np.empty((B, F, N + 1), dtype=np.complex128)
    for f in range(F):
        out[:, f] = np.fft.rfft(gyp[:, f * hop:f * hop + n] * wa, axis=-1)
    out[..., 0] = 0.5 * out[..., 0].real
    out[..., N] = 0.5 * out[..., N].real
    return out


def impulse_closed_form(shape, t0):
    """gX (F, n / 2 + 1) for gy = delta[t0] of one entry: c_k g w[j] / (n E[t0 + c]) e^(-2 pi i j k / n), j = t0 + c - f hop, in
    every frame that covers it"""
    _, F, n, hop, centred, wname, wl, _, normalized = shape
    N, c = n // 2, (n // 2 if centred else 0)
    w = table_of(wname, wl, n)
    w = np.ones(n) if w is None else w
    g = float(np.float32(np.sqrt(float(n)))) if normalized else 1.0
    E = envelope(w, n, hop, F)
    ck = np.full(N + 1, 2.0)
    ck[0] = ck[N] = 1.0
    k = np.arange(N + 1)
    out = np.zeros((F, N + 1), dtype=np.complex128)
    for f in range(F):
        j = t0 + c - f * hop
        if 0 <= j < n:
            out[f] = ck * g * w[j] / (n * E[t0 + c]) * np.exp(-2j * np.pi * j * k / n)
    out[:, 0] = out[:, 0].real
    out[:, N] = out[:, N].real
    return out


def mdct_matrix(n):
    """the dense cosine matrix of an MDCT of n coefficients: C[k, j] = cos(pi / n (j + 1/2 + n/2)(k + 1/2)), (n, 2n)"""
    j = np.arange(2 * n)[None, :]
    k = np.arange(n)[:, None]
    return np.cos(np.pi / n * (j + 0.5 + n / 2.0) * (k + 0.5))


def mdct_model(x, n, w, scale):
    """X[b, f, k] = scale sum_j w[j] x~[(f - 1) n + j] C[k, j], x (B, T) with zeros outside [0, T); torch or numpy float64.
    Returns (B, F, n), F = ceil(T / n) + 1."""
    tor = isinstance(x, torch.Tensor)
    B, T = x.shape
    F = (T + n - 1) // n + 1
    C = mdct_matrix(n) * np.asarray(w)[None, :]
    if tor:
        xp = torch.zeros((B, (F + 1) * n), dtype=torch.float64)
        xp[:, n:n + T] = x
        frames = torch.stack([xp[:, f * n:f * n + 2 * n] for f in range(F)], dim=1)
        return scale * frames @ torch.from_numpy(C).T
    xp = np.zeros((B, (F + 1) * n))
    xp[:, n:n + T] = x
    frames = np.stack([xp[:, f * n:f * n + 2 * n] for f in range(F)], axis=1)
    return scale * frames @ C.T


def imdct_model(X, n, w, gain, length):
    """y[b, t] = gain sum over the two frames f that cover t of w[j] sum_k X[b, f, k] C[k, j], j = t - (f - 1) n; X (B, F, n)
    torch or numpy float64.  Returns (B, length)."""
    tor = isinstance(X, torch.Tensor)
    B, F, _ = X.shape
    C = mdct_matrix(n) * np.asarray(w)[None, :]
    y = gain * (X @ (torch.from_numpy(C) if tor else C))  # (B, F, 2n)
    out = torch.zeros((B, (F + 1) * n), dtype=torch.float64) if tor else np.zeros((B, (F + 1) * n))
    for f in range(F):
        out[:, f * n:f * n + 2 * n] = out[:, f * n:f * n + 2 * n] + y[:, f]
    return out[:, n:n + length]
