"""The ray-binning arithmetic of csrc/mrt_bin.hip restated in numpy, twice.

The float32 restatement (bin_items, bin_valid, bin_key, bin_key_inst, and expect() on top of
them) follows the device code operation by operation: every float32 operation is rounded on
its own (the library is built with -ffp-contract=off), sums run left to right, fmaxf returns
the number when the other argument is NaN, the float -> int conversion truncates and
saturates (NaN -> 0), and the count of bin_items is taken through a 64-bit intermediate.

bin_key_f64 is independent of it: float64, a real division, floor, no mirrored order of
operations.  tests/test_bin_rays.py holds the first to the second away from cell edges, and
the device to the first everywhere."""
import numpy as np

F = np.float32
INVALID = 0xFFFF
_M64 = (1 << 64) - 1


def bin_items(n, n_dev=None, mul1=1, sub=0, cap1=0xFFFFFFFF, mul2=1):
    """The number of slots the passes look at."""
    if n_dev is None:
        return int(n)
    v = (int(n_dev) * int(mul1)) & _M64   # uint32 * uint32 in a uint64
    v = v - sub if v > sub else 0
    v = min(v, int(cap1))
    v = (v * int(mul2)) & _M64
    return v if v < n else int(n)


def bin_valid(items, nrays=None, m=1):
    """Per slot i < items: i % m < nrays[i / m] (no nrays: every slot)."""
    i = np.arange(items, dtype=np.int64)
    if nrays is None:
        return np.ones(items, bool)
    return (i % m) < np.asarray(nrays, np.int64)[i // m]


def _cell(x, n):
    """bin_cell: (int)fminf(fmaxf(x, 0), n - 1); NaN -> 0."""
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(x.astype(F), F(0)), F(n - 1)).astype(np.int64)


def _morton(cx, cy, cz, obits):
    mort = np.zeros_like(cx)
    for b in range(obits):
        mort |= (((cx >> b) & 1) << (3 * b)) | (((cy >> b) & 1) << (3 * b + 1)) | (((cz >> b) & 1) << (3 * b + 2))
    return mort


def dir_cells(d, dbits):
    """(iu, iv): the octahedral cell of each direction, lower hemisphere folded."""
    d = np.asarray(d, F)
    nd = 1 << dbits
    with np.errstate(all="ignore"):
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        inv_s = np.where(s > 0, F(1) / s, F(0)).astype(F)
        u, v = dx * inv_s, dy * inv_s
        fold = dz < 0
        u2 = (F(1) - np.abs(v)) * np.where(u >= 0, F(1), F(-1))
        v2 = (F(1) - np.abs(u)) * np.where(v >= 0, F(1), F(-1))
        u, v = np.where(fold, u2, u).astype(F), np.where(fold, v2, v).astype(F)
        iu = _cell((u * F(0.5) + F(0.5)) * F(nd), nd)
        iv = _cell((v * F(0.5) + F(0.5)) * F(nd), nd)
    return iu, iv


def bin_key(o, d, lo, inv, dbits, obits):
    """The plain key: ((iu << dbits | iv) << 3 obits) | Morton(cx, cy, cz)."""
    o = np.asarray(o, F)
    lo, inv = np.asarray(lo, F), np.asarray(inv, F)
    iu, iv = dir_cells(d, dbits)
    no = 1 << obits
    with np.errstate(all="ignore"):
        c = [_cell((o[:, a] - lo[a]) * inv[a], no) for a in range(3)]
    return (((iu << dbits) | iv) << (3 * obits)) | _morton(c[0], c[1], c[2], obits)


def _sat_cell4(x):
    """min(3, max(0, (int)x)) with a saturating conversion: NaN -> 0, beyond int -> the end."""
    with np.errstate(all="ignore"):
        x = np.where(np.isnan(x), F(0), x)
        return np.clip(np.trunc(np.clip(x, -4.0, 8.0)), 0, 3).astype(np.int64)


def bin_key_inst(o, d, lo, inv, m, hits, hit_base, inst_class, n_world, inst_cell=None, inst_inv=None):
    """Instance-major keys (dbits = obits = 2): slot i's pixel is i / m."""
    o = np.asarray(o, F)
    n = len(o)
    hits = np.asarray(hits, F).reshape(-1, 4)
    prim = hits[:, 3].copy().view(np.int32).astype(np.int64)[np.arange(n) // m]
    plain = bin_key(o, d, lo, inv, 2, 2)
    hit_base = np.asarray(hit_base, np.int64)
    # the last instance whose hit_base <= prim (instance 0 when there is none)
    inst = np.maximum(0, np.searchsorted(hit_base, prim, side="right") - 1)
    dirc = plain >> 6
    if inst_cell is None:
        key = (1 << 11) | (np.asarray(inst_class, np.int64)[inst] << 4) | dirc
    else:
        cell = np.asarray(inst_cell, F).reshape(-1, 2, 4)
        M = np.asarray(inst_inv, F).reshape(-1, 3, 4)[inst]
        c0, c1 = cell[inst, 0], cell[inst, 1]
        with np.errstate(all="ignore"):
            p = [((M[:, r, 0] * o[:, 0] + M[:, r, 1] * o[:, 1]) + M[:, r, 2] * o[:, 2]) + M[:, r, 3] for r in range(3)]
            c = [_sat_cell4((p[a] - c0[:, a]) * c1[:, a]) for a in range(3)]
        morton = (c[0] & 1) | (c[1] & 1) << 1 | (c[2] & 1) << 2 | (c[0] >> 1) << 3 | (c[1] >> 1) << 4 | (c[2] >> 1) << 5
        key = (1 << 11) | np.where(c0[:, 3] != 0, 1 << 10, 0) | (morton << 4) | dirc
    return np.where(prim < n_world, plain, key)


def expect(o, d, *, n_dev=None, mul1=1, sub=0, cap1=0xFFFFFFFF, mul2=1, nrays=None, m=1, lo=(0, 0, 0), inv=(1, 1, 1),
           dbits=2, obits=2, hits=None, hit_base=None, inst_class=None, n_world=0, inst_cell=None, inst_inv=None, **_):
    """What the three launches leave: items, the valid mask and the key of every slot < items,
    the per-bin counts.  Takes the keyword arguments of miro.bin_rays."""
    o = np.asarray(o, F).reshape(-1, 4)
    d = np.asarray(d, F).reshape(-1, 4)
    items = bin_items(len(o), n_dev, mul1, sub, cap1, mul2)
    valid = bin_valid(items, nrays, m)
    if hits is None:
        bits = 2 * dbits + 3 * obits
        keys = bin_key(o[:items], d[:items], lo, inv, dbits, obits)
    else:
        bits = 12
        keys = bin_key_inst(o[:items], d[:items], lo, inv, m, hits, hit_base, inst_class, n_world, inst_cell, inst_inv)
    keys = np.where(valid, keys, INVALID)
    counts = np.bincount(keys[valid], minlength=1 << bits)
    return {"items": items, "valid": valid, "keys": keys, "bits": bits, "counts": counts}


# ---------------------------------------------------------------- the independent float64 statement
def bin_key_f64(o, d, lo, inv, dbits, obits):
    """(key, scaled): the plain key in float64 with floor and a real division, and the five
    scaled coordinates (su, sv, cx, cy, cz) before they are cut to cells.  Finite inputs and
    non-zero directions only."""
    o, d = np.asarray(o, np.float64)[:, :3], np.asarray(d, np.float64)[:, :3]
    nd, no = 1 << dbits, 1 << obits
    uv = d[:, :2] / np.abs(d).sum(axis=1, keepdims=True)
    sign = np.where(uv >= 0, 1.0, -1.0)
    folded = (1.0 - np.abs(uv[:, ::-1])) * sign
    uv = np.where(d[:, 2:3] < 0, folded, uv)
    suv = (uv + 1.0) / 2.0 * nd
    sc = (o - np.asarray(lo, np.float64)) * np.asarray(inv, np.float64)
    ij = np.clip(np.floor(suv), 0, nd - 1).astype(np.int64)
    c = np.clip(np.floor(sc), 0, no - 1).astype(np.int64)
    mort = np.zeros(len(o), np.int64)
    for a in range(3):   # axis a's bit b is bit 3 b + a of the code
        for b in range(obits):
            mort += ((c[:, a] // (1 << b)) % 2) * 8 ** b * 2 ** a
    key = (ij[:, 0] * nd + ij[:, 1]) * 8 ** obits + mort
    return key, np.concatenate([suv, sc], axis=1)
