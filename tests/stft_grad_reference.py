"""What the STFT gradient tests share: the shapes, the windows, the torch.stft reference on the CPU in fp64, and an fp64 numpy
model of the adjoint exactly as the kernel computes it (the synthesis table with its sign, the doubled DC / Nyquist bins, the
ascending-frame overlap-add, the edge strips, the fold and the zero tail), which tests/test_stft_grad_host.py holds against
torch.autograd over torch.stft."""
import numpy as np
import torch

# (B, T, n, hop, centre, window): the smallest at which each mechanism can go wrong
SMALL_SHAPES = [
    (3, 50, 16, 4, "reflect", "hann"),
    (3, 53, 16, 5, "reflect", None),       # odd hop, rectangular
    (3, 50, 16, 4, "constant", "hann"),
    (3, 50, 16, 3, None, "hamming"),
    (2, 47, 16, 16, None, "hann"),         # hop = n: no carry; L < T: a zero tail
    (2, 41, 32, 7, "reflect", "hann"),
    (2, 9, 16, 4, "reflect", "hann"),      # n / 2 = T - 1: the two folds overlap
]


def window_of(name, n):
    """periodic windows, as torch.hann_window / torch.hamming_window; None: rectangular"""
    if name is None:
        return None
    a = {"hann": 0.5, "hamming": 0.54}[name]
    return a - (1.0 - a) * np.cos(2.0 * np.pi * np.arange(n) / n)


def frames_of(T, n, hop, centre):
    return 1 + (T // hop if centre else (T - n) // hop)


def torch_stft(x, n, hop, centre, w, normalized=False):
    """torch.stft of a (B, T) tensor with a full-length window table ``w`` (numpy float64, or None)"""
    wt = torch.ones(n, dtype=x.dtype, device=x.device) if w is None else torch.as_tensor(w, dtype=x.dtype, device=x.device)
    kw = dict(center=centre is not None, return_complex=True, window=wt, normalized=normalized)
    if centre:
        kw["pad_mode"] = centre
    return torch.stft(x, n, hop, **kw)  # (B, bins, F)


def adjoint_model(x_arg, mult, mode, w, n, hop, T, centre, gain=1.0):
    """The adjoint as the kernel computes it, in float64.  ``x_arg`` complex (B, F, n / 2 + 1), frames-major: the gradient
    (mode 1) or X (modes 2, 3, with the real ``mult``).  Returns (gx (B, T), out (B, T) as the launch leaves it with NaN where it
    writes nothing, edge (B, 2, n / 2) likewise or None)."""
    x_arg = np.asarray(x_arg, dtype=np.complex128)
    B, F, _ = x_arg.shape
    N = n // 2
    c = N if centre else 0
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    g = x_arg.copy()
    if mode == 2:
        g = g * mult
    elif mode == 3:
        r = np.abs(g)
        g = g * np.where(r == 0, 0.0, mult / np.where(r == 0, 1.0, r))
    g[..., 0] = 2.0 * g[..., 0].real   # the imaginary parts of bins 0 and N drop out
    g[..., N] = 2.0 * g[..., N].real
    y = np.fft.irfft(g, n=n, axis=-1) * n  # what the passes leave: unscaled
    sign = np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    ws = sign * (gain if mode == 2 else 0.5 * gain) * w  # the synthesis table, the sign of the conjugation folded in
    L = n + hop * (F - 1)
    assert L <= T + 2 * c
    gxp = np.zeros((B, L))
    for f in range(F):  # ascending frames; the kernel's LDS holds sign * y
        gxp[:, f * hop:f * hop + n] += ws * (sign * y[:, f])
    out = np.full((B, T), np.nan)
    cov = min(T, L - c)
    out[:, :cov] = gxp[:, c:c + cov]
    edge = None
    if centre == "reflect":
        edge = np.full((B, 2, N), np.nan)
        edge[:, 0] = gxp[:, :c]
        e = max(0, min(c, L - c - T))
        edge[:, 1, :e] = gxp[:, c + T:c + T + e]
    gx = out.copy()
    gx[:, cov:] = 0.0  # the zero tail
    if edge is not None:
        gx[:, 1:c + 1] += edge[:, 0, ::-1]
        e = max(0, min(c, L - c - T))
        if e:
            gx[:, T - 1 - e:T - 1] += edge[:, 1, :e][:, ::-1]
    return gx, out, edge
