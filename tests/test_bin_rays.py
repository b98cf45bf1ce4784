"""Ray binning (csrc/mrt_bin.hip) looked at directly: the keys, the scan and the scatter of the
three launches, through the probe entry mrt_debug_bin_rays (miro.bin_rays), against the numpy
restatement in tests/bin_reference.py.

The frame tests of tests/test_binning.py prove that a binned order changes no pixel, that is
that `perm` is some permutation of the valid slots; a constant key, swapped direction cells, a
binary search off by one or an over-count would pass them all and only cost speed.  Here every
case asserts, against the restatement: the key of every valid slot, 0xFFFF in every invalid
one, the caller's fill past the item count; the total; the cursors after the scatter (the
inclusive running count of the bins); and that `perm` lists exactly the valid slots, bin by
bin, with the caller's fill behind them.  Order within a bin follows the atomics and is not
asserted.

On the CPU: the float32 restatement against an independent float64 one, and the probe's own
refusals (made before any device call)."""
import ctypes as C

import numpy as np
import pytest

import bin_reference as R
import miro
from miro import _lib

F = np.float32
KEYS_FILL, PERM_FILL = 0xABCD, 0xDEADBEEF   # no key (> 4095, not 0xFFFF), no slot
PAIRS = [(1, 0), (0, 1), (2, 2), (5, 0), (3, 2), (6, 0), (0, 4)]   # 2, 3, 10, 10, 12, 12, 12 bits
BOX_LO, BOX_EXT = (0.25, 0.5, 1.0), (6.0, 5.0, 4.5)


def box_inv(obits):   # bin_args' scale of the scene box (csrc/mrt_device.hip)
    return tuple(F(1 << obits) / F(e) for e in BOX_EXT)


def random_rays(n, seed):
    """Origins uniform in (-1, 7)^3 (inside and around the box), normal directions."""
    rng = np.random.default_rng(seed)
    o, d = np.empty((n, 4), F), np.empty((n, 4), F)
    o[:, :3] = rng.uniform(-1.0, 7.0, (n, 3))
    d[:, :3] = rng.standard_normal((n, 3))
    o[:, 3], d[:, 3] = 1e30, np.nan   # w is unused
    return o, d


def rays_of(origins, dirs):
    o, d = np.zeros((len(origins), 4), F), np.zeros((len(dirs), 4), F)
    o[:, :3], d[:, :3] = np.asarray(origins, F), np.asarray(dirs, F)
    return o, d


def check(o, d, key_bits=True, **kw):
    """One probe call; every assertion of the module docstring.  key_bits=False: the keys are
    only held to their range (the sort is then checked on the device's own keys)."""
    try:
        got = miro.bin_rays(o, d, keys_fill=KEYS_FILL, perm_fill=PERM_FILL, **kw)
    except miro.MRTError as e:
        if "MRT_ERR_HIP" in str(e):   # the device reported an error: launch nothing more on it
            pytest.exit("mrt_debug_bin_rays: %s" % e, returncode=3)
        raise
    exp = R.expect(o, d, **kw)
    items, valid, K = exp["items"], exp["valid"], 1 << exp["bits"]
    assert got["bits"] == exp["bits"]
    keys = got["keys"].astype(np.int64)
    # keys
    assert np.all(keys[items:] == KEYS_FILL), "keys past the item count were written"
    assert np.all(keys[:items][~valid] == R.INVALID), "an invalid slot without the invalid key"
    if key_bits:
        bad = np.flatnonzero(keys[:items] != exp["keys"])
        assert bad.size == 0, "slot %d: key %#x, expected %#x (%d differ)" % (bad[0], keys[bad[0]], exp["keys"][bad[0]], bad.size)
    else:
        assert np.all(keys[:items][valid] < K)
    want = keys[:items]
    slots = np.flatnonzero(valid)
    counts = np.bincount(want[slots], minlength=K)
    total = slots.size
    # total and cursors
    hist = got["hist"].astype(np.int64)
    assert hist[K] == total, "total %d, %d valid slots" % (hist[K], total)
    assert np.array_equal(hist[:K], np.cumsum(counts)), "cursors after the scatter"
    # perm
    perm = got["perm"].astype(np.int64)
    assert np.all(perm[total:] == PERM_FILL), "perm past the total was written"
    p = perm[:total]
    assert np.array_equal(np.sort(p), slots), "perm is not the valid slots"
    kp = want[p]
    assert np.all(np.diff(kp) >= 0), "keys along perm decrease"
    assert np.array_equal(p[np.lexsort((p, kp))], slots[np.argsort(want[slots], kind="stable")]), "a bin's segment holds other slots"
    return got, exp


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("dbits,obits", PAIRS)
def test_float32_restatement_agrees_with_float64(dbits, obits):
    """20,000 seeded rays per width: the step-by-step float32 restatement and the independent
    float64 one give the same key wherever the five scaled coordinates (su, sv, cx, cy, cz,
    before truncation) lie further than 1e-4 from an integer; under 1 % of the rays are
    excluded (0.08-0.14 % expected: 5 coordinates x 2e-4 / 1, less the clamped ones)."""
    o, d = random_rays(20000, 1000 + 16 * dbits + obits)
    k32 = R.bin_key(o, d, BOX_LO, box_inv(obits), dbits, obits)
    k64, scaled = R.bin_key_f64(o, d, BOX_LO, box_inv(obits), dbits, obits)
    if dbits == 0:
        scaled = scaled[:, 2:]    # one direction cell: su, sv decide nothing
    if obits == 0:
        scaled = scaled[:, :2]
    near = np.any(np.abs(scaled - np.rint(scaled)) <= 1e-4, axis=1)
    print("(%d, %d): %.3f %% excluded, %d disagree outside the margin" % (dbits, obits, 100 * near.mean(), np.sum((k32 != k64) & ~near)))
    assert near.mean() < 0.01
    assert np.array_equal(k32[~near], k64[~near])
    assert len(np.unique(k32)) > (1 << (2 * dbits + 3 * obits)) // 2   # the rays reach most bins


def test_items_restatement_by_hand():
    """bin_items on the forms the call sites use, worked by hand."""
    assert R.bin_items(600) == 600
    assert R.bin_items(600, 100, mul2=3) == 300
    assert R.bin_items(600, 250, mul2=3) == 600
    assert R.bin_items(240, 7, 9, 20, 40, 6) == 240     # 63 - 20 = 43, capped to 40, x 6
    assert R.bin_items(240, 7, 9, 30, 40, 6) == 198     # 33 x 6
    assert R.bin_items(240, 7, 9, 63, 40, 6) == 0
    assert R.bin_items(240, 7, 9, 100, 40, 6) == 0
    assert R.bin_items(240, 477218589, 9, 2, 30, 6) == 180   # 2^32 + 5 - 2, capped to 30 (a 32-bit product: 3 x 6)


def probe(**kw):
    a = {k: np.zeros(16, np.uint8) for k in ("o", "d", "keys", "hist", "perm")}
    P = _lib.mrt_bin_probe()
    P.n, P.m, P.grid, P.dbits, P.obits = 1, 1, 1, 2, 2
    P.mul1, P.cap1, P.mul2 = 1, 0xFFFFFFFF, 1
    for k, v in a.items():
        setattr(P, k, v.ctypes.data)
    for k, v in kw.items():
        setattr(P, k, v)
    rc = miro.lib().mrt_debug_bin_rays(C.byref(P))
    del a
    return rc, miro.lib().mrt_last_error().decode()


def test_probe_refusals():
    """The probe's own refusals, each MRT_ERR_INVALID with its text, made before any device call."""
    L = miro.lib()
    assert L.mrt_debug_bin_rays(None) == -1
    for k in ("o", "d", "keys", "hist", "perm"):
        assert probe(**{k: None}) == (-1, "null ray-bin probe array"), k
    assert probe(m=0) == (-1, "ray-bin probe: m must be at least 1")
    for g in (0, -1, 1025):
        assert probe(grid=g) == (-1, "ray-bin probe: grid must be 1..1024"), g
    for n in (1 << 31, 0xFFFFFFFF):
        assert probe(n=n) == (-1, "ray-bin probe: fewer than 2^31 rays"), n
    t = np.zeros(64, np.uint16)   # table stand-ins (never read: refused first)
    p = t.ctypes.data
    assert probe(hits=p, hit_base=p, inst_class=p, n_inst=1, inst_cell=p) == (-1, "ray-bin probe: inst_cell needs the instance matrices")
    for kw in (dict(hit_base=p, n_inst=1), dict(inst_class=p, n_inst=1), dict(hit_base=p, inst_class=p, n_inst=0), dict()):
        assert probe(hits=p, **kw) == (-1, "ray-bin probe: hits need the instance tables"), kw
    t[2] = 128
    assert probe(hits=p, hit_base=p, inst_class=p, n_inst=3) == (-1, "ray-bin probe: inst_class above 127")


# ------------------------------------------------------------------------------------ (a) sizes and grids
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 2, 7])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 1000, 2049])
def test_sizes_and_grids(n, grid):
    o, d = random_rays(n, 7 + n)
    check(o, d, grid=grid, lo=BOX_LO, inv=box_inv(2))


@pytest.mark.gpu
@pytest.mark.parametrize("n,grid", [(100, 8), (5000, 3)])
def test_empty_and_ragged_block_ranges(n, grid):
    """100 rays on 8 workgroups: seven have an empty range.  5000 on 3: 1792 per block, the last 1416."""
    o, d = random_rays(n, 11 + n)
    check(o, d, grid=grid, lo=BOX_LO, inv=box_inv(2))


# ------------------------------------------------------------------------------------ (b) key edges
# dbits = obits = 2, lo = 0, inv = 1: direction cell = min(3, floor(2 (t + 1))) of the octahedral
# u and v, origin cell = min(3, max(0, floor(x))) per axis; every coordinate dyadic, so each
# step of the device's arithmetic is exact and the keys below are worked by hand.
AXES = [((1, 0, 0), (3, 2)), ((-1, 0, 0), (0, 2)), ((0, 1, 0), (2, 3)), ((0, -1, 0), (2, 0)), ((0, 0, 1), (2, 2)),
        ((0, 0, -1), (3, 3))]   # -z: u = v = 0 folds to (1, 1)
# (sx, sy, sz)/3: |u| = |v| = 1/3 above the equator (cells 2 / 1), 2/3 folded below it (cells 3 / 0)
DIAGONALS = [((sx, sy, sz), ((2 if sx > 0 else 1, 2 if sy > 0 else 1) if sz > 0 else (3 if sx > 0 else 0, 3 if sy > 0 else 0)))
             for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
EDGES = [((-1, 0, 0.0), (0, 2)), ((-0.5, 0, 0.5), (1, 2)), ((0.0, 0, 1), (2, 2)), ((0.5, 0, 0.5), (3, 2)), ((1, 0, -0.0), (3, 2)),
         ((0, -1, -0.0), (2, 0)), ((0, -0.5, 0.5), (2, 1)), ((0, 0.5, 0.5), (2, 3)), ((0, 1, 0.0), (2, 3)),
         ((3, 1, 0.0), (3, 2)), ((3, 1, -0.0), (3, 2)),            # u = 0.75, v = 0.25; -0.0 is not below 0: no fold
         ((0.25, 0.25, -0.5), (3, 3)),                              # folds to (0.75, 0.75)
         ((0.5, 0, -0.5), (3, 3)), ((-0.5, 0, -0.5), (0, 3)),      # fold to (1, 0.5) and (-1, 0.5): clamp and cell edge
         ((0, -0.5, -0.5), (3, 0)), ((-0.25, 0.25, -0.5), (0, 3))]
INF, NAN = float("inf"), float("nan")
ORIGINS = [((0, 0, 0), 0), ((1, 0, 0), 1), ((0, 1, 0), 2), ((0, 0, 1), 4), ((2, 0, 0), 8), ((0, 2, 0), 16), ((0, 0, 2), 32),
           ((3, 0, 0), 9), ((4, 4, 4), 63), ((1, 2, 3), 1 | 16 | 4 | 32), ((0.5, 1.5, 2.5), 2 | 32), ((3.5, 3.5, 3.5), 63),
           ((-1, -0.5, -1e30), 0), ((1e30, 0, 0), 9), ((NAN, 1, NAN), 2), ((INF, -INF, 0), 9), ((-0.0, 4.5, 1e-30), 2 | 16)]
ODD_DIRS = [(0, 0, 0), (NAN, NAN, NAN), (INF, 0, 0), (-INF, 1, 2), (0, INF, -INF), (INF, INF, INF), (NAN, 1, 0), (1, NAN, -1),
            (1, 1, NAN), (0, 0, NAN), (-0.0, -0.0, -0.0), (3e38, 3e38, 3e38), (-3e38, 3e38, -3e38)]


@pytest.mark.gpu
def test_key_edges_by_hand():
    dirs = AXES + DIAGONALS + EDGES
    o = [(1, 2, 3)] * len(dirs) + [p for p, _ in ORIGINS]
    d = [v for v, _ in dirs] + [(0, 0, 1)] * len(ORIGINS)
    hand = [((iu << 2 | iv) << 6) | 53 for _, (iu, iv) in dirs] + [((2 << 2 | 2) << 6) | mort for _, mort in ORIGINS]
    o, d = rays_of(o, d)
    assert np.array_equal(R.bin_key(o, d, (0, 0, 0), (1, 1, 1), 2, 2), hand), "the restatement against the hand-worked keys"
    got, _ = check(o, d, grid=1)
    assert np.array_equal(got["keys"], hand)


@pytest.mark.gpu
def test_odd_directions_and_flat_box_land_in_valid_keys():
    """Zero, NaN, infinite and mixed directions, each at every origin of ORIGINS: a key like any
    other (the restatement's, NaN -> cell 0).  Then the flat box, inv = 0: origin cell 0 whatever
    the origin (NaN and inf included: NaN -> 0)."""
    o, d = rays_of([p for p, _ in ORIGINS for _ in ODD_DIRS], [v for _ in ORIGINS for v in ODD_DIRS])
    got, _ = check(o, d, grid=2)
    assert np.all(got["keys"] < 1 << 10)
    dirs = AXES + DIAGONALS
    o, d = rays_of([ORIGINS[i % len(ORIGINS)][0] for i in range(len(dirs))], [v for v, _ in dirs])
    got, _ = check(o, d, grid=1, inv=(0, 0, 0))
    assert np.array_equal(got["keys"], [(iu << 2 | iv) << 6 for _, (iu, iv) in dirs])
    got, _ = check(o, d, grid=1, inv=(0, 1, 0), lo=(0, 0, 7))   # flat in x and z only: bits 1 and 4 of the Morton code
    assert np.all(got["keys"] & 0b101101 == 0) and np.any(got["keys"] & 0b010010)


@pytest.mark.gpu
def test_denormal_directions_keep_the_sort_invariants():
    """Directions of denormal magnitude: 1 / s overflows or is flushed depending on the
    denormal mode, so only the key range and the sort invariants are asserted."""
    rng = np.random.default_rng(5)
    o, d = random_rays(500, 5)
    d[:, :3] = (rng.integers(-50, 51, (500, 3)) * 1e-42).astype(F)
    d[::7, :3] *= F(1e3)
    check(o, d, key_bits=False, grid=2, lo=BOX_LO, inv=box_inv(2))


# ------------------------------------------------------------------------------------ (c) widths
@pytest.mark.gpu
@pytest.mark.parametrize("dbits,obits", PAIRS)
def test_key_widths(dbits, obits):
    """2, 3, 10 and 12 bits: the scan with one bin per thread (fewer bins than threads included)
    and with four."""
    o, d = random_rays(3000, 50 + 16 * dbits + obits)
    _, exp = check(o, d, grid=2, dbits=dbits, obits=obits, lo=BOX_LO, inv=box_inv(obits))
    assert np.count_nonzero(exp["counts"]) > (1 << exp["bits"]) // 3


@pytest.mark.gpu
@pytest.mark.parametrize("dbits,obits", [(0, 0), (7, 0), (0, 5), (3, 3)])
def test_bad_key_widths_are_refused(dbits, obits):
    o, d = random_rays(10, 1)
    with pytest.raises(miro.MRTError, match="MRT_ERR_INVALID: bad ray-bin key bits"):
        miro.bin_rays(o, d, dbits=dbits, obits=obits)


def octahedral_centre(iu, iv, nd):
    """A direction in the middle of direction cell (iu, iv): the octahedral map inverted."""
    u, v = (iu + 0.5) / nd * 2 - 1, (iv + 0.5) / nd * 2 - 1
    z = 1 - abs(u) - abs(v)
    if z < 0:
        u, v = (1 - abs(v)) * (1 if u >= 0 else -1), (1 - abs(u)) * (1 if v >= 0 else -1)
    return (u, v, z)


@pytest.mark.gpu
def test_one_bin_holds_every_ray():
    o, d = rays_of([(1.5, 2.5, 0.5)] * 5000, [(0.3, -0.2, 0.9)] * 5000)
    _, exp = check(o, d, grid=3)
    assert np.count_nonzero(exp["counts"]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("dbits,obits", [(6, 0), (3, 2), (0, 4)])
def test_4096_bins_with_one_ray_each(dbits, obits):
    """The key map inverted on cell centres: every bin of a 12-bit key exactly once, shuffled."""
    nd, no = 1 << dbits, 1 << obits
    dirs = [octahedral_centre(iu, iv, nd) for iu in range(nd) for iv in range(nd)]
    cells = [(x + 0.5, y + 0.5, z + 0.5) for x in range(no) for y in range(no) for z in range(no)]
    o, d = rays_of([c for _ in dirs for c in cells], [v for v in dirs for _ in cells])
    order = np.random.default_rng(3).permutation(4096)
    o, d = o[order], d[order]
    _, exp = check(o, d, grid=4, dbits=dbits, obits=obits)
    assert np.array_equal(exp["counts"], np.ones(4096, np.int64))


@pytest.mark.gpu
def test_first_bin_empty_last_bin_full():
    o, d = rays_of([(3.5, 3.5, 3.5)] * 40 + [(1.5, 0.5, 2.5)] * 30, [(0, 0, -1)] * 40 + [(1, -1, 1)] * 30)
    _, exp = check(o, d, grid=2)
    assert exp["counts"][0] == 0 and exp["counts"][1023] == 40 and exp["counts"].sum() == 70


# ------------------------------------------------------------------------------------ (d) validity and counts
def ray_counts(px, m, seed):
    c = np.random.default_rng(seed).integers(0, m + 1, px).astype(np.uint8)
    c[:m + 1] = np.arange(m + 1)   # every count 0..m occurs
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3, 7])
def test_ray_counts_per_pixel(m):
    px = 150
    for n in (px * m, px * m - (m - 1)):   # the last pixel complete, and cut short
        o, d = random_rays(n, 20 + m)
        _, exp = check(o, d, grid=2, nrays=ray_counts(px, m, m), m=m, lo=BOX_LO, inv=box_inv(2))
        assert 0 < exp["valid"].sum() < n or m == 1
    o, d = random_rays(px * m, 21)
    _, exp = check(o, d, grid=2, nrays=np.zeros(px, np.uint8), m=m)   # every slot invalid: total 0
    assert exp["valid"].sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_dev", [0, 100, 200, 250])
@pytest.mark.parametrize("m", [1, 3])
def test_device_count_of_a_chain_level(n_dev, m):
    """B.n_dev = the level's count, B.mul2 = m (csrc/mrt_device.hip, the chain levels): below,
    equal to and above the capacity of 200 pixels, and 0.  Slots past the items keep the fills."""
    px = 200
    o, d = random_rays(px * m, 30 + m)
    _, exp = check(o, d, grid=2, n_dev=n_dev, mul2=m, nrays=ray_counts(px, m, 9), m=m, lo=BOX_LO, inv=box_inv(2))
    assert exp["items"] == min(n_dev, px) * m


@pytest.mark.gpu
@pytest.mark.parametrize("n_dev,sub,cap1,items", [(7, 20, 40, 240), (7, 30, 40, 198), (7, 62, 40, 6), (7, 63, 40, 0), (7, 100, 40, 0),
                                                   (7, 0, 5, 30), (477218589, 2, 30, 180)])
def test_device_count_of_an_adaptive_pass(n_dev, sub, cap1, items):
    """The adaptive form: units = min(cap1, n_dev * 9 - sub), items = units * num_paths * m with
    num_paths = 2, m = 3 on 240 slots: sub below, at and above the product, cap1 binding and
    not, and a product past 2^32 (2^32 + 5: a 32-bit product would give 3 units, not 30)."""
    o, d = random_rays(240, 40)
    _, exp = check(o, d, grid=2, n_dev=n_dev, mul1=9, sub=sub, cap1=cap1, mul2=6, nrays=ray_counts(80, 3, 4), m=3,
                   lo=BOX_LO, inv=box_inv(2))
    assert exp["items"] == items


# ------------------------------------------------------------------------------------ (e) instance-major keys
N_WORLD = 10
HIT_BASE = [10, 25, 26, 90]       # (instances 1 and 2 adjacent: hit_base[2] - 1 is hit_base[1])
CLASSES = [0, 127, 1, 64]
# hit id -> instance (None: a world hit or a miss, the plain key), worked by hand
PRIMS = [(-1, None), (0, None), (9, None), (10, 0), (11, 0), (24, 0), (25, 1), (26, 2), (27, 2), (89, 2), (90, 3), (91, 3),
         (1000, 3), (2 ** 31 - 1, 3), (-2 ** 31, None)]


def pixel_hits(prims):
    h = np.zeros((len(prims), 4), F)
    h[:, :3] = 0.5
    h[:, 3] = np.asarray(prims, np.int64).astype(np.int32).view(F)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3])
def test_instance_major_keys(m):
    """1 << 11 | class << 4 | direction cell for a pixel whose hit lies on an instance, the plain
    key (below 1 << 11) otherwise; the m rays of a pixel share its hit."""
    px = len(PRIMS)
    o, d = random_rays(px * m, 60 + m)
    got, _ = check(o, d, grid=2, m=m, lo=BOX_LO, inv=box_inv(2), hits=pixel_hits([p for p, _ in PRIMS]), hit_base=HIT_BASE,
                   inst_class=CLASSES, n_world=N_WORLD)
    keys = got["keys"].astype(np.int64)
    plain = R.bin_key(o, d, BOX_LO, box_inv(2), 2, 2)
    assert np.all(plain < 1 << 11)
    for i, k in enumerate(keys):
        inst = PRIMS[i // m][1]
        if inst is None:
            assert k == plain[i], (i, hex(k))
        else:
            assert k >> 11 == 1 and (k >> 4) & 127 == CLASSES[inst] and k & 15 == plain[i] >> 6, (i, hex(k), inst)


@pytest.mark.gpu
def test_instance_major_keys_of_one_instance():
    """n_inst = 1, its first hit id above n_world: ids from n_world on are its own."""
    prims = [9, 10, 11, 12, 13, 500]
    o, d = random_rays(len(prims), 63)
    got, _ = check(o, d, grid=1, hits=pixel_hits(prims), hit_base=[12], inst_class=[77], n_world=10)
    assert list(got["keys"] >> 11) == [0, 1, 1, 1, 1, 1]
    assert np.all((got["keys"][1:] >> 4) & 127 == 77)


@pytest.mark.gpu
def test_instance_major_refusals():
    o, d = random_rays(6, 64)
    tables = dict(hits=pixel_hits([10] * 6), hit_base=HIT_BASE, inst_class=CLASSES, n_world=N_WORLD)
    for dbits, obits in ((3, 2), (2, 1), (6, 0)):
        with pytest.raises(miro.MRTError, match="instance-major ray-bin keys need dbits = obits = 2"):
            miro.bin_rays(o, d, dbits=dbits, obits=obits, **tables)
    with pytest.raises(miro.MRTError, match="hits need the instance tables"):
        miro.bin_rays(o, d, hits=pixel_hits([10] * 6), hit_base=HIT_BASE)
    with pytest.raises(miro.MRTError, match="m must be at least 1"):
        miro.bin_rays(o, d, m=0, **tables)


# ------------------------------------------------------------------------------------ (f) object-space keys
# world -> object matrices (3 x 4, dyadic): a quarter turn about z with a translation, a
# non-uniform scale with a translation, a zero scale (x and z collapse), the identity
INST_INV = [[[0, 1, 0, -2], [-1, 0, 0, 3], [0, 0, 1, 0.5]],
            [[2, 0, 0, -1], [0, 0.5, 0, 0.25], [0, 0, 4, 0]],
            [[0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0]],
            [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]]
# per instance (BLAS box lo, BLAS bit), (4 / extent, 0); instance 2's box is flat in z
INST_CELL = [[[-1, -1, -1, 0], [2, 2, 2, 0]], [[0, 0, 0, 1], [1, 0.5, 2, 0]], [[0, 0, 0, 0], [1, 1, 0, 0]],
             [[-2, -2, -2, 1], [1, 1, 1, 0]]]


def object_morton(cx, cy, cz):
    return (cx & 1) | (cy & 1) << 1 | (cz & 1) << 2 | (cx >> 1) << 3 | (cy >> 1) << 4 | (cz >> 1) << 5


@pytest.mark.gpu
def test_object_space_keys():
    """1 << 11 | BLAS bit << 10 | Morton code of the origin's cell in its instance's BLAS box
    << 4 | direction cell.  By hand: origins on, inside and outside each box; by the restatement:
    random origins around the boxes.  A NaN or 1e30 after the transform is converted to int
    before the clamp: the key of a saturating conversion (NaN -> 0)."""
    # (instance, world origin) -> object cell, by hand
    hand = [(0, (0, 0, 0), (0, 3, 3)),            # object (y - 2, 3 - x, z + 0.5) = (-2, 3, 0.5): below, above, 1.5 * 2 = 3
            (0, (-3, -1, -1.5), (0, 3, 0)),       # object (-3, 6, -1): z on lo
            (0, (2.75, 1.5, -0.5), (1, 2, 2)),    # object (-0.5, 0.25, 0): 0.5 * 2, 1.25 * 2, 1 * 2: inside, z on a cell edge
            (0, (2, 3, 0.5), (3, 3, 3)),          # object (1, 1, 1): on hi, 4 clamped to 3
            (1, (0.5, -0.5, 0), (0, 0, 0)),       # object (2x - 1, y / 2 + 0.25, 4z) = (0, 0, 0): on lo
            (1, (2.5, 15.5, 0.5), (3, 3, 3)),     # object (4, 8, 2): on hi
            (1, (1.25, 7.5, 0.3125), (1, 2, 2)),  # object (1.5, 4, 1.25): 1.5, 4 / 2, 1.25 * 2
            (2, (9, 2.5, 9), (1, 2, 0)),          # object (1, 2.5, 0): x and z collapsed, the flat axis' scale 0
            (3, (-2, 1, 1.5), (0, 3, 3)),         # the identity: (0, 3, 3.5)
            (3, (1e30, -1e30, 5e29), (3, 0, 3)),  # far outside: a saturating conversion, then the clamp
            (3, (INF, 1, 1), (3, 0, 0)),          # x inf; y and z hold 0 * inf = NaN -> 0
            (0, (NAN, 0, 0), (0, 0, 0)),          # every row holds a product with NaN
            (1, (1e30, -1e30, 3e38), (3, 0, 3))]  # z overflows to inf in the transform
    bases = [10, 20, 30, 40]
    rng = np.random.default_rng(8)
    n_rand = 400
    inst = [h[0] for h in hand] + list(rng.integers(0, 4, n_rand))
    o, d = random_rays(len(inst), 66)
    o[:len(hand), :3] = np.asarray([h[1] for h in hand], F)
    o[len(hand):, :3] = rng.uniform(-4, 4, (n_rand, 3)).round(2)
    prims = [bases[i] + 3 for i in inst]
    prims[-5:] = [2] * 5   # world hits among them: plain keys
    kw = dict(hits=pixel_hits(prims), hit_base=bases, inst_class=[0, 0, 0, 0], n_world=10, inst_cell=INST_CELL, inst_inv=INST_INV)
    got, exp = check(o, d, grid=2, **kw)
    keys = got["keys"].astype(np.int64)
    plain = R.bin_key(o, d, (0, 0, 0), (1, 1, 1), 2, 2)
    for i, (ins, _, cell) in enumerate(hand):
        want = 1 << 11 | int(INST_CELL[ins][0][3]) << 10 | object_morton(*cell) << 4 | int(plain[i] >> 6)
        assert exp["keys"][i] == want, ("the restatement against the hand-worked key", i, hex(exp["keys"][i]), hex(want))
        assert keys[i] == want, (i, hex(keys[i]), hex(want))
    assert np.all(keys[-5:] == plain[-5:]) and np.all(keys[:-5] >> 11 == 1)
    assert np.array_equal((keys[:-5] >> 10) & 1, [int(INST_CELL[i][0][3]) for i in inst[:-5]])
    # the object-space cell is not the world cell (two bits per axis: the same Morton layout): most codes differ
    assert np.mean(plain[len(hand):-5] & 63 != (keys[len(hand):-5] >> 4) & 63) > 0.5
