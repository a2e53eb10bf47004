"""mifft -- MI355X-native batched N-D radix-N FFT (drop-in for the GPU hot path of
martinvuyk/hackathon-fft).  See include/mifft.h for the C ABI, DESIGN.md for the kernels.
"""
from ._lib import MifftError, LIB_PATH, EXPORTS  # noqa: F401
from .api import (  # noqa: F401
    FLAG_DCT,
    FLAG_DCT_ND,
    FLAG_DCT_ORTHO,
    FLAG_ISTFT,
    FLAG_STFT,
    FLAG_STFT_CENTER_REFLECT,
    FLAG_STFT_CENTER_ZEROS,
    FLAG_STFT_HOP,
    DeviceContext,
    GPUTest,
    Plan,
    clear_plan_cache,
    dct,
    dctn,
    estimate_best_bases,
    estimate_best_bases_nd,
    fft,
    fftn,
    idct,
    idctn,
    ifftn,
    irfftn,
    istft,
    istft_length,
    istft_schedule,
    ordered_bases,
    plan_fft,
    plan_istft,
    plan_stft,
    reduce_dims,
    rfftn,
    stft,
    stft_frames,
    time_fft,
)

__all__ = [
    "DeviceContext", "GPUTest", "Plan", "clear_plan_cache", "MifftError", "estimate_best_bases", "estimate_best_bases_nd",
    "fft", "fftn", "ifftn", "irfftn", "ordered_bases", "plan_fft", "reduce_dims", "rfftn", "time_fft", "dct", "idct",
    "FLAG_DCT", "FLAG_DCT_ORTHO", "FLAG_DCT_ND", "dctn", "idctn",
    "FLAG_STFT", "FLAG_STFT_CENTER_REFLECT", "FLAG_STFT_CENTER_ZEROS", "FLAG_STFT_HOP", "plan_stft", "stft", "stft_frames",
    "FLAG_ISTFT", "plan_istft", "istft", "istft_length", "istft_schedule",
]
