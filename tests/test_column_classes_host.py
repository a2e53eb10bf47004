"""The column-tile classes of tests/test_gpu_column_classes.py, as far as they need no device: the class table, the shapes the
sweep runs (pure functions, held here to what they promise), the byte counts that put a twiddle table into LDS or into global
memory, and where the paired-column DCT / DST tiles accept a column length and where they refuse one, through
mifft_plan_create without a device.

choose_config(n, cols=true, ..) (csrc/kernels_jit.cpp) derives from the column length n, the float type and the stride the radix
list (one to four passes; past 8192 / 4096 tile elements at the default tile a three-pass re-choice with radices up to 16 / 10),
the tile (16 / 8 columns, 32 / 64 at a stride that is a multiple of it while n * tile stays within 4096 / 2048 elements, halved
down to 2 while the tile exceeds 16384 / 8192 elements -- four passes: 8192 / 4096 -- or 136 KiB), the threads (one per 20 / 10
tile elements, 128 to 512), the one-wave shape of a single radix (64 columns, 64 threads), and where the twiddle table lives.

"Accepted" is `rc in (0, -10)`: planned where there is a device, MIFFT_ERR_NO_DEVICE -- the answer of a request that passed
every host check -- where there is none."""
import numpy as np
import pytest

from test_dctn_host import DCT_ND, KEEP, UNSUPPORTED
from test_dctn_host import _create as dctn_create
from test_dst_host import TAG2, dst2_by_dct, ref_dstn
from test_dst_host import _create as dst_create

ACCEPTED = (0, -10)
LDS_TABLE_BYTES = 156 * 1024  # choose_config: the table stays in LDS while tile and table fit this

# (dtype, n, pairs): (radices, tile, threads, where the twiddle table lives) -- what choose_config answers, and why the length is
# here.  pairs None: the stride is left to the sweep (an odd number of pairs, no wide tile); a number: that many pairs of real
# columns (kept elements of the complex plan), a multiple of the wide tile.
# Where the twiddle table lives is not visible through a plan.  It follows from choose_config's byte count: the table stays in
# LDS while (n * tile + sum over the passes k >= 1 of P_k (R_k - 1)) complex elements fit 156 KiB = 159744 bytes (P_k: the
# product of the radices before pass k).  fp32 4096: (16384 + 4080) * 8 = 163712 bytes; fp32 4092: (16368 + 4081) * 8 = 163592;
# fp64 2023: (8092 + 2016) * 16 = 161728; fp64 3375: (6750 + 3360) * 16 = 161760; fp64 4092: (8184 + 4081) * 16 = 196240: global
# memory.  fp64 3332: (6664 + 3318) * 16 = 159712 bytes, 32 short of the limit: the longest fp64 column with its table in LDS;
# fp32 2025: (16200 + 2016) * 8 = 145728 and fp32 1001: (16016 + 994) * 8 = 136080: in LDS, as every other key.
CLASSES = {
    ("f32", 7, None): ((7,), 64, 64, "lds"),                # odd prime, one butterfly per column, one wave
    ("f32", 8, None): ((8,), 64, 64, "lds"),                # even single radix
    ("f32", 31, None): ((31,), 64, 64, "lds"),              # the largest register radix
    ("f32", 15, None): ((3, 5), 16, 128, "lds"),            # odd n, two passes
    ("f32", 81, None): ((3, 3, 3, 3), 16, 128, "lds"),      # four passes at the full tile
    ("f32", 169, None): ((13, 13), 16, 256, "lds"),         # 256 threads
    ("f32", 625, None): ((5, 5, 5, 5), 8, 256, "lds"),      # first halving (four-pass cap of 8192 elements)
    ("f32", 1001, None): ((7, 11, 13), 16, 512, "lds"),     # odd, 128128-byte tile; the chooser's own three passes
    ("f32", 1250, None): ((5, 5, 5, 10), 4, 256, "lds"),    # tile 4, four passes
    ("f32", 2025, None): ((9, 15, 15), 8, 512, "lds"),      # three-pass re-choice, odd n
    ("f32", 2401, None): ((7, 7, 7, 7), 2, 256, "lds"),     # tile 2
    ("f32", 3375, None): ((15, 15, 15), 4, 512, "lds"),     # three-pass re-choice, tile 4
    ("f32", 4095, None): ((5, 7, 9, 13), 2, 512, "lds"),    # longest four-pass column, odd
    ("f32", 4092, None): ((11, 12, 31), 4, 512, "global"),  # twiddles in global memory, radix 31
    ("f32", 4096, None): ((16, 16, 16), 4, 512, "global"),  # the limit; twiddles in global memory
    ("f32", 49, 128): ((7, 7), 64, 256, "lds"),             # 64-wide tile
    ("f32", 81, 64): ((3, 3, 3, 3), 32, 256, "lds"),        # 32-wide tile (64 columns would exceed 4096 elements)
    ("f64", 7, None): ((7,), 64, 64, "lds"),                # odd prime, one wave
    ("f64", 31, None): ((31,), 64, 64, "lds"),              # the largest register radix
    ("f64", 49, None): ((7, 7), 8, 128, "lds"),             # default fp64 tile
    ("f64", 66, None): ((6, 11), 8, 128, "lds"),            # radix above the fp64 soft cap
    ("f64", 625, None): ((5, 5, 5, 5), 4, 256, "lds"),      # first halving
    ("f64", 729, None): ((9, 9, 9), 8, 512, "lds"),         # three-pass re-choice
    ("f64", 1024, None): ((4, 4, 8, 8), 4, 512, "lds"),     # four passes, tile 4
    ("f64", 2023, None): ((7, 17, 17), 4, 512, "global"),   # tile 4, twiddles in global memory
    ("f64", 2025, None): ((5, 5, 9, 9), 2, 512, "lds"),     # tile 2, odd
    ("f64", 2048, None): ((4, 8, 8, 8), 2, 512, "lds"),     # the longest four-pass fp64 column
    ("f64", 3332, None): ((14, 14, 17), 2, 512, "lds"),     # the longest column whose table still fits LDS
    ("f64", 3375, None): ((15, 15, 15), 2, 512, "global"),  # twiddles in global memory
    ("f64", 4092, None): ((11, 12, 31), 2, 512, "global"),  # the longest accepted fp64 column
    ("f64", 49, 64): ((7, 7), 32, 256, "lds"),              # fp64 wide tile
    ("f64", 81, 32): ((3, 3, 3, 3), 16, 256, "lds"),        # fp64 wide tile, next step down
}
KEYS = list(CLASSES)
KINDS = ["dct2", "dct3", "dst2", "dst3"]
ORTHO_KEYS = [("f32", 2401, None), ("f32", 4096, None), ("f64", 2025, None), ("f64", 4092, None)]
# the lengths of the table that the precompiled column tables hold (fast_table_gen_cols*.inc): a plain complex column pass of
# these takes the table's kernel and its own shape, not choose_config's
PRECOMPILED = [("f32", 4096, None), ("f64", 1024, None), ("f64", 2048, None)]
BATCH = 2


def key_id(key):
    t, n, pairs = key
    return f"{t}-{n}" + ("" if pairs is None else f"-{pairs}pairs")


def table_bytes(key):
    """tile and twiddle table in bytes, recomputed from the radices: choose_config's count"""
    t, n, _ = key
    radices, tile, _, _ = CLASSES[key]
    entries, p = 0, 1
    for k, r in enumerate(radices):
        if k >= 1:
            entries += p * (r - 1)
        p *= r
    assert p == n
    return (n * tile + entries) * (16 if t == "f64" else 8)


# ---- the shapes of the sweep (pure) ------------------------------------------------------------------------------------------

def pairs_of(key):
    """pairs of real columns of the paired-column cases: two full tiles and a ragged one of a single pair; a wide key: its own
    count, two full tiles (a ragged one would change the stride and with it the tile)"""
    return 2 * CLASSES[key][1] + 1 if key[2] is None else key[2]


def real_width(key):
    """W of the (B, n, W, 1) tensor: the stride of the transformed dim in reals"""
    return 2 * pairs_of(key)


def kept_width(key):
    """I of the (B, n, I, 2) tensor of the kept-dim complex plan: two full tiles and a ragged column, odd (no wide tile), and
    at least 128 bytes of kept elements (below that axes.cpp takes the interleaved block tile); a wide key: its own count"""
    t, _, pairs = key
    if pairs is not None:
        return pairs
    return max(2 * CLASSES[key][1] + 1, 9 if t == "f64" else 17)


def test_the_shapes_are_what_the_sweep_promises():
    for key in KEYS:
        t, n, pairs = key
        radices, tile, threads, _ = CLASSES[key]
        esz = 16 if t == "f64" else 8
        W, I = real_width(key), kept_width(key)
        assert W % 2 == 0 and W >= 4 and W == 2 * pairs_of(key), key      # an even stride of at least 4 reals
        assert BATCH * n * W <= 2 * 4096 * 18, key
        if pairs is None:
            assert pairs_of(key) == 2 * tile + 1, key                      # two full tiles and a single pair
            assert -(-pairs_of(key) // tile) == 3 and pairs_of(key) % tile == 1, key
            assert I % 2 == 1 and I * esz >= 128 and I >= 2 * tile + 1, key  # odd: no wide tile; a column tile, not ILV
            assert -(-I // tile) >= 3 or len(radices) == 1, key
            wides = (32, 16) if t == "f64" else (64, 32)
            assert all(pairs_of(key) % w and I % w for w in wides), key
        else:
            assert pairs % tile == 0 and pairs // tile == 2 and I == pairs, key  # a multiple of the wide tile: two full tiles
            assert tile > (8 if t == "f64" else 16) and n * tile <= (2048 if t == "f64" else 4096), key
            assert I * esz >= 128, key
    assert len(KEYS) == 32 and len({(t, n) for t, n, p in KEYS if p is None}) == 28
    assert all(k in CLASSES for k in ORTHO_KEYS + PRECOMPILED)
    assert max(BATCH * n * real_width((t, n, p)) for t, n, p in KEYS) == 2 * 4096 * 18


def test_the_byte_counts_that_decide_lds_or_global():
    """recomputed from the radices for every key; the figures of the table's comment"""
    for key in KEYS:
        where = "lds" if table_bytes(key) <= LDS_TABLE_BYTES else "global"
        assert where == CLASSES[key][3], (key, table_bytes(key))
        t, n, _ = key
        assert n * CLASSES[key][1] * (16 if t == "f64" else 8) <= 136 * 1024, key  # the tile itself: choose_config's cap
    assert LDS_TABLE_BYTES == 159744
    for key, want in ((("f32", 4096, None), 163712), (("f32", 4092, None), 163592), (("f64", 2023, None), 161728),
                      (("f64", 3375, None), 161760), (("f64", 4092, None), 196240), (("f64", 3332, None), 159712),
                      (("f32", 2025, None), 145728), (("f32", 1001, None), 136080)):
        assert table_bytes(key) == want, (key, table_bytes(key))
    assert 4096 * 4 * 8 + 4080 * 8 == 163712 and 1001 * 16 * 8 == 128128


def test_the_thread_counts_follow_from_the_tile():
    """one thread per 20 (fp64: 10) tile elements, a power of two from 128 to 512; a single radix: one wave"""
    for key in KEYS:
        t, n, _ = key
        radices, tile, threads, _ = CLASSES[key]
        if len(radices) == 1:
            assert (tile, threads) == (64, 64), key
            continue
        per = 10 if t == "f64" else 20
        want = 1
        while want < -(-n * tile // per):
            want *= 2
        assert threads == max(128, min(512, want)), key


# ---- acceptance, without a device --------------------------------------------------------------------------------------------

def _types(t):
    return dict(in_dtype=1, out_dtype=1) if t == "f64" else {}


def create_cols(t, n, W, kind="dct2"):
    """a paired-column plan of n points at a stride of W reals, the last dim kept: (status, reason)"""
    inverse = kind.endswith("3")
    if kind.startswith("dst"):
        return dst_create([n, W], bases=(TAG2,), inverse=inverse, flags=DCT_ND | KEEP(1), batch=BATCH, **_types(t))
    return dctn_create([n, W], inverse=inverse, flags=DCT_ND | KEEP(1), batch=BATCH, **_types(t))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_every_class_of_the_sweep_is_accepted(key, kind):
    rc, why = create_cols(key[0], key[1], real_width(key), kind)
    assert rc in ACCEPTED, (key, kind, rc, why)


@pytest.mark.parametrize("kind", KINDS)
def test_the_boundaries_of_both_types(kind):
    rc, why = create_cols("f32", 4096, 18, kind)
    assert rc in ACCEPTED, (rc, why)
    rc, why = create_cols("f32", 4098, 18, kind)
    assert rc == UNSUPPORTED and "4096" in why, (rc, why)
    rc, why = create_cols("f64", 4092, 10, kind)
    assert rc in ACCEPTED, (rc, why)
    for n in (4095, 4096):
        rc, why = create_cols("f64", n, 10, kind)
        assert rc == UNSUPPORTED and "column configuration" in why, (n, rc, why)
    for t in ("f32", "f64"):
        rc, why = create_cols(t, 74, 10, kind)
        assert rc == UNSUPPORTED and "prime factor above 32" in why, (t, rc, why)


FP64_REFUSED_INSIDE = (2058, 2080, 2100, 2401, 4000)
FP64_ACCEPTED_INSIDE = (2023, 3332, 3375, 4080)


@pytest.mark.parametrize("kind", KINDS)
def test_fp64_columns_the_four_pass_preference_refuses_today(kind):
    """NOT a contract, the state of choose_config: choose_radices prefers four passes of radices up to 8 (10), a four-pass fp64
    tile holds at most 4096 elements, so from 2058 points on such a list is refused even at a tile of 2 -- and nothing retries
    with three passes, which would fit (2080 = 10 x 13 x 16 at a tile of 2: 66 KB).  157 lengths between 2058 and 4096, these
    five among them; their neighbours whose best list has three passes are accepted, and fp32 accepts all nine.  A chooser
    that retries makes this test fail: move its lengths to the accepted ones then (follow-up)."""
    for n in FP64_REFUSED_INSIDE:
        rc, why = create_cols("f64", n, 10, kind)
        assert rc == UNSUPPORTED and "column configuration" in why, (n, rc, why)
    for n in FP64_ACCEPTED_INSIDE:
        rc, why = create_cols("f64", n, 10, kind)
        assert rc in ACCEPTED, (n, rc, why)
    for n in FP64_REFUSED_INSIDE + FP64_ACCEPTED_INSIDE:
        rc, why = create_cols("f32", n, 18, kind)
        assert rc in ACCEPTED, (n, rc, why)


# ---- the sine reference of the long columns ----------------------------------------------------------------------------------

def test_the_cosine_route_of_the_sine_reference_is_the_sine_matrix():
    """ref_dstn goes the sine matrix up to 1080 points and sign, reversal and the cosine reference beyond; the two at 15 and 16
    points along a middle axis, both directions, both norms"""
    rng = np.random.default_rng(1516)
    for n in (15, 16):
        x = rng.standard_normal((2, n, 6))
        for inverse in (False, True):
            for norm in (None, "ortho"):
                want = ref_dstn(x, (1,), inverse, norm)
                got = np.moveaxis(dst2_by_dct(np.moveaxis(x, 1, -1), norm, inverse), -1, 1)
                assert np.abs(got - want).max() < 1e-12, (n, inverse, norm)
