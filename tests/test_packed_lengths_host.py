"""Where the packed-row family accepts a row length and where it refuses one, through mifft_plan_create without a device.

One rule (include/mifft.h, MIFFT_FLAG_HALF_SPECTRUM): n / 2 needs a packed configuration whose row tile fits 96 KiB of LDS.
An fp32 row of 16384 points is 64 KiB; an fp64 row is n / 2 complex doubles, so the longest has 12288 points (exactly 96 KiB),
and 12320, the next length whose half is smooth, is refused.  The inverse STFT keeps a carry of n reals beside the tile: in fp64
tile and carry fill the CU's 160 KiB at 10240 points, and 10290, the next smooth length, is refused for the carry.  The GPU side
of both boundaries is tests/test_gpu_packed_lengths.py.

"Accepted" is `rc in (0, -10)`: planned where there is a device, MIFFT_ERR_NO_DEVICE -- the answer of a request that passed
every host check -- where there is none."""
import pytest

from test_dct4_host import _create as dct4_create
from test_dct_host import _create as dct_create
from test_half_spectrum_host import _create as half_create
from test_imdct_host import _create as imdct_create
from test_istft_host import HOP, ISTFT
from test_istft_host import _create as istft_create
from test_mdct_host import _create as mdct_create
from test_stft_host import STFT
from test_stft_host import _create as stft_create

UNSUPPORTED = -15
ACCEPTED = (0, -10)


def _types(f64):
    return dict(in_dtype=1, out_dtype=1) if f64 else {}


# every kernel of the family but the inverse STFT: (n, fp64?) -> (status, reason)
PLAIN = {
    "dct2": lambda n, f64: dct_create([n], **_types(f64)),
    "dct3": lambda n, f64: dct_create([n], inverse=True, **_types(f64)),
    "dct4": lambda n, f64: dct4_create([n], **_types(f64)),
    "r2c": lambda n, f64: half_create([n], comps=1, inverse=False, **_types(f64)),
    "c2r": lambda n, f64: half_create([n], comps=2, inverse=True, **_types(f64)),
    "stft": lambda n, f64: stft_create([4 * n, n], flags=STFT | HOP(n // 4), **_types(f64)),
    "mdct": lambda n, f64: mdct_create(4 * n, n, **_types(f64)),
    "imdct": lambda n, f64: imdct_create(2 * n, 5, n, **_types(f64)),
}


def _istft(n, f64):
    """5 rectangular frames every n // 4 samples, n output samples"""
    return istft_create([n, 5, n], flags=ISTFT | HOP(n // 4), **_types(f64))


@pytest.mark.parametrize("kernel", sorted(PLAIN))
def test_fp64_rows_go_up_to_12288_points(kernel):
    rc, why = PLAIN[kernel](12288, True)
    assert rc in ACCEPTED, (kernel, rc, why)
    rc, why = PLAIN[kernel](12320, True)  # 6160 = 2^4 * 5 * 7 * 11 is smooth: only the tile is too large
    assert rc == UNSUPPORTED and "packed" in why, (kernel, rc, why)


def test_the_fp64_inverse_stft_goes_up_to_10240_points():
    rc, why = _istft(10240, True)
    assert rc in ACCEPTED, (rc, why)
    rc, why = _istft(10290, True)  # 5145 = 3 * 5 * 7^3: a tile of 80.4 KiB plans as rows, but not beside its carry
    assert rc == UNSUPPORTED and "carry" in why, (rc, why)
    rc, why = PLAIN["c2r"](10290, True)
    assert rc in ACCEPTED, (rc, why)
    rc, why = _istft(12288, True)
    assert rc == UNSUPPORTED and "carry" in why, (rc, why)


@pytest.mark.parametrize("kernel", sorted(PLAIN) + ["istft"])
def test_fp32_rows_go_up_to_16384_points(kernel):
    rc, why = (_istft if kernel == "istft" else PLAIN[kernel])(16384, False)
    assert rc in ACCEPTED, (kernel, rc, why)
