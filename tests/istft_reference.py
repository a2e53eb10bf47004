"""What the inverse STFT tests share: the shapes, random spectrograms, and the fp64 reference (numpy irfft, window, overlap-add
in ascending frame order, division by the overlap-added squared window), which tests/test_istft_host.py holds against
torch.istft on the CPU."""
import functools

import numpy as np

# (B, F, n, hop, window, centred, length); the last FP32_ONLY rows run in fp32 only
FP32_ONLY = 2
SHAPES = [
    (5, 29, 16, 3, "hann", True, None),        # odd hop, F no multiple of a tile
    (5, 29, 16, 3, "hamming", False, None),    # the same, uncentred
    (3, 7, 16, 16, None, False, None),         # hop == n: no carry
    (3, 7, 16, 12, "hamming", False, None),    # hop > n / 2
    (4, 1, 16, 4, "hamming", False, None),     # one frame
    (4, 2, 64, 1, "hamming", False, None),     # F < K
    (2, 300, 128, 1, "hamming", False, None),  # K - 1 = 127 > TILE: two warm-up tiles once a run starts mid-entry
    (2, 9, 30, 7, "hamming", True, 50),        # odd N = 15, length= shorter than covered
    (3, 41, 400, 160, "hann", True, 6400),
    (2, 33, 1024, 256, "hann", True, 8000),
    (1, 5, 16384, 4096, "hann", True, None),   # one frame per tile, tile + carry fill LDS: the twiddle table in global memory
    (1, 5, 16000, 4000, "hann", True, None),   # the same with radices 10x10x10x8: 512 threads where the plain rows take 1024
]


def window_of(name, n):
    """periodic windows, as torch.hann_window / torch.hamming_window; None: rectangular"""
    if name is None:
        return None
    a = {"hann": 0.5, "hamming": 0.54}[name]
    return a - (1.0 - a) * np.cos(2.0 * np.pi * np.arange(n) / n)


def spectrogram(B, F, n, seed=0):
    """random complex128 (B, F, n // 2 + 1), frames leading; the imaginary parts of bins 0 and n / 2 are NOT zero"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, F, n // 2 + 1)) + 1j * rng.standard_normal((B, F, n // 2 + 1))


def istft_length(F, n, hop, centred):
    return n + hop * (F - 1) - (2 * (n // 2) if centred else 0)


def istft_reference(X, n, hop, window, centred, length=None, gain=1.0):
    """X complex (B, F, n // 2 + 1) -> float64 (B, T)"""
    X = np.asarray(X, dtype=np.complex128)
    B, F, _ = X.shape
    w = np.ones(n) if window is None else np.asarray(window, dtype=np.float64)
    y = np.fft.irfft(X, n=n, axis=-1) * (gain * w)
    L = n + hop * (F - 1)
    acc = np.zeros((B, L))
    env = np.zeros(L)
    for f in range(F):
        acc[:, f * hop:f * hop + n] += y[:, f]
        env[f * hop:f * hop + n] += w * w
    c = n // 2 if centred else 0
    T = istft_length(F, n, hop, centred) if length is None else length
    assert c + T <= L and np.abs(env[c:c + T]).min() > 1e-11
    return acc[:, c:c + T] / env[c:c + T]


def rel_l2_blocks(got, ref, hop):
    """relative L2 error over blocks of max(hop, 16) consecutive samples, the maximum over blocks and batch entries"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    blk = max(int(hop), 16)
    worst = 0.0
    for s in range(0, ref.shape[-1], blk):
        d = np.linalg.norm(got[:, s:s + blk] - ref[:, s:s + blk], axis=-1)
        r = np.linalg.norm(ref[:, s:s + blk], axis=-1)
        worst = max(worst, float((d / r).max()))
    return worst
