"""Transforms over a subset of the dims (MIFFT_FLAG_KEEP_DIM, torch `dim=`): the ABI constants, every refusal that needs no
device (the C library checks before it looks for a HIP device) and the host-side `dim` reduction of the wrappers."""
import ctypes
import os
import re

import pytest
import torch

import hackathon_fft_amd as mf
from hackathon_fft_amd import _lib
from conftest import ROOT

BAD_DIM, BAD_BASES, UNSUPPORTED, NO_DEVICE = -2, -5, -15, -10
HALF = 2


def KEEP(d):
    return 1 << (8 + d)


def _create(dims, *, comps=2, inverse=False, in_dtype=0, out_dtype=0, flags=0, bases=None):
    L = _lib.lib()
    h = ctypes.c_void_p()
    c_dims = (ctypes.c_int64 * len(dims))(*dims)
    c_flat = c_len = None
    if bases is not None:
        flat = [b for bs in bases for b in bs]
        c_flat = (ctypes.c_uint32 * max(1, len(flat)))(*flat)
        c_len = (ctypes.c_int32 * len(dims))(*[len(bs) for bs in bases])
    rc = L.mifft_plan_create(ctypes.byref(h), 0, in_dtype, out_dtype, len(dims), c_dims, 3, comps, int(inverse),
                             c_flat, c_len, flags)
    if rc == 0:
        L.mifft_plan_destroy(h)
    return rc, L.mifft_last_error().decode()


def test_keep_flag_is_declared():
    h = open(os.path.join(ROOT, "include", "mifft.h")).read()
    assert re.search(r"#define\s+MIFFT_FLAG_KEEP_DIM\(d\)\s+\(\(uint32_t\)1u\s*<<\s*\(8\s*\+\s*\(d\)\)\)", h)
    assert re.search(r"#define\s+MIFFT_FLAG_KEEP_MASK\s+0x3F00u", h)
    assert mf.api.FLAG_KEEP_DIM(0) == 0x100 and mf.api.FLAG_KEEP_DIM(5) == 0x2000 and mf.api.FLAG_KEEP_MASK == 0x3F00


def test_keep_bit_beyond_ndim_is_bad_dim():
    rc, why = _create([64, 4], flags=KEEP(2))
    assert rc == BAD_DIM and "ndim" in why
    rc, why = _create([64], flags=KEEP(5))
    assert rc == BAD_DIM


def test_every_dim_kept_is_bad_dim():
    rc, why = _create([64, 4], flags=KEEP(0) | KEEP(1))
    assert rc == BAD_DIM and "no dimension to transform" in why
    rc, why = _create([64], flags=KEEP(0))
    assert rc == BAD_DIM and "no dimension to transform" in why


def test_faithful_stages_with_a_mask_is_unsupported():
    rc, why = _create([64, 4], flags=1 | KEEP(1))
    assert rc == UNSUPPORTED and "FAITHFUL" in why


def test_bases_of_a_kept_dim_are_refused():
    rc, why = _create([64, 4], flags=KEEP(1), bases=[[2], [2]])
    assert rc == BAD_BASES and "dimension 1" in why
    # an empty list for the kept dim passes validation and reaches the device lookup
    if not torch.cuda.is_available():
        rc, _ = _create([64, 4], flags=KEEP(1), bases=[[2], []])
        assert rc == NO_DEVICE


def test_existing_size_check_stays_for_kept_dims():
    rc, _ = _create([64, 1], flags=KEEP(1))
    assert rc == BAD_DIM


def test_unrouted_masked_plans_are_unsupported_before_the_device():
    rc, why = _create([8192, 3], flags=KEEP(1))  # a strided dim beyond one column tile
    assert rc == UNSUPPORTED and "dimension 0" in why
    rc, why = _create([4, 32768], flags=KEEP(0))  # an innermost dim beyond one row launch
    assert rc == UNSUPPORTED and "dimension 1" in why
    rc, why = _create([4, 16384], flags=KEEP(0), out_dtype=1, in_dtype=1)  # fp64 complex rows end at 8192 points (128 KiB)
    assert rc == UNSUPPORTED
    rc, why = _create([64, 32, 4], comps=1, flags=HALF | KEEP(2))  # half spectrum of a kept last dim
    assert rc == UNSUPPORTED and "last dimension kept" in why


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device answer of valid requests")
@pytest.mark.parametrize("dims,flags,comps,inverse", [
    ([1024, 4], KEEP(1), 2, False),
    ([64, 7, 64], KEEP(1), 2, True),
    ([5, 128], KEEP(0), 1, False),
    ([16384, 2][::-1], KEEP(1), 2, False),   # (2, 16384): dim 0 at stride 16384 ... kept
    ([4096, 8], KEEP(1), 1, False),
    ([64, 7, 32], HALF | KEEP(1), 1, False),
    ([64, 7, 32], HALF | KEEP(0), 2, True),
])
def test_valid_masked_requests_reach_the_device_lookup(dims, flags, comps, inverse):
    rc, why = _create(dims, comps=comps, inverse=inverse, flags=flags)
    assert rc == NO_DEVICE, why


def test_lane_offset_check_skips_kept_dims():
    # dim 0 kept: 2^20 x 2^13 would span 2^33 elements as a strided transformed dim; kept, it is only carried through
    rc, why = _create([1 << 20, 1 << 13], flags=KEEP(0))
    if not torch.cuda.is_available():
        assert rc == NO_DEVICE, why
    rc, why = _create([1 << 20, 1 << 13], flags=KEEP(1))
    assert rc in (-9, UNSUPPORTED), why


# ---- the Python `dim` reduction (pure host logic) ----

R = mf.reduce_dims


def test_reduce_single_dim_and_negative_index():
    assert R((4, 100, 3), 1) == ((4, 100, 3), (1,))
    assert R((4, 100, 3), -2) == ((4, 100, 3), (1,))
    assert R((4, 100, 3), (-1,)) == ((400, 3), (1,))


def test_reduce_dim0_adds_a_batch_of_one():
    assert R((4, 100, 3), 0) == ((1, 4, 300), (1,))
    assert R((6, 8), (0, 1)) == ((1, 6, 8), (1, 2))


def test_reduce_drops_size_one_dims():
    assert R((4, 1, 6), (1,)) is None           # only a length-1 transform: the identity
    assert R((4, 5, 1, 6, 7), (0, 3)) == ((1, 4, 5, 6, 7), (1, 3))
    assert R((1, 9, 1, 5), (1, 3)) == ((1, 9, 5), (1, 2))


def test_reduce_merges_adjacent_kept_dims():
    assert R((2, 64, 3, 5, 64), (1, 4)) == ((2, 64, 15, 64), (1, 3))
    assert R((2, 3, 4, 8, 5, 6), (3,)) == ((24, 8, 30), (1,))
    assert R((100, 480, 640, 3), (1, 2)) == ((100, 480, 640, 3), (1, 2))


def test_reduce_all_but_first_is_the_plain_layout():
    assert R((7, 16, 32), (1, 2)) == ((7, 16, 32), (1, 2))


def test_reduce_empty_dim_is_identity():
    assert R((4, 5, 6), ()) is None


def test_reduce_too_many_dims_after_merging():
    with pytest.raises(mf.MifftError) as e:
        R((2, 3, 4, 5, 6, 7, 8, 9), (1, 3, 5, 7))
    assert e.value.status == -1
    # the same rank with adjacent kept dims merges below the limit
    assert R((2, 3, 4, 5, 6, 7, 8, 9), (1, 2, 3, 4)) == ((2, 3, 4, 5, 6, 504), (1, 2, 3, 4))


def test_reduce_bad_dims():
    with pytest.raises(mf.MifftError):
        R((4, 5), 2)
    with pytest.raises(mf.MifftError):
        R((4, 5), (1, -1))


def test_plan_axes_map_to_keep_bits():
    assert mf.api._keep_flags(5, None) == 0
    assert mf.api._keep_flags(5, (1, 3)) == KEEP(1)
    assert mf.api._keep_flags(4, (2,)) == KEEP(0)
    with pytest.raises(mf.MifftError):
        mf.api._keep_flags(4, (3,))
