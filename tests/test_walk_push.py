"""The push block of traverse_impl (csrc/mrt_kernels.h) on the frame kernel: the four-entry
LDS push on both sides of its `sp + 4 <= 16` boundary, the entry-by-entry path into the
spill column (also in a tile whose lanes take different sides of the boundary), a stack
overflow reported by the walk itself (from the camera rays' walk, and from the shadow rays'
walk alone) and the frame after it, each under walk_exit 0/1 x walk_latch 0/1 x
scalar_nodes 0/7; and the 4-GiB limit of the node and leaf arrays that the walks' 32-bit
byte offsets rest on.

The hierarchies are imported (mrt_scene_bvh_import), which the oracle cannot take, but they
all hold the same single triangle: what a ray hits does not depend on the hierarchy above
the triangle, so the oracle's frame of the plain scene is the expected frame -- float and
8-bit RGB, hit records and the shadow-ray count, bit for bit -- and every covered pixel hits
prim 0 on z = -5."""
import ctypes as C
import itertools

import numpy as np
import pytest

import miro
from helpers import bits, camera, scene_pair, tuned
from miro import _lib

W, H = 24, 16   # six 8x8 tiles (one wave each): the triangle in the middle, background around it
TRI = (np.array([(-1, -1, -5), (1, -1, -5), (0, 1, -5)], np.float32), np.array([(0, 0, 1)], np.float32),
       np.array([(0, 1, 2)], np.uint32), np.array([(0, 0, 0)], np.uint32))
CAM = dict(eye=(0.0, 0.0, 0.0), lookAt=(0.0, 0.0, -1.0), up=(0, 1, 0), fov=30.0)
LIGHT = (1.0, 2.0, 0.0)          # in front of the triangle: every walk crosses boxes that hold everything
LIGHT_PX = (10.0, 0.0, -4.5)     # far to the +x side: the shadow rays leave along +x, through SIDE_BOX
LIGHT_NX = (-10.0, 0.0, -4.5)    # its mirror image: they leave along -x and never meet SIDE_BOX
EMPTY = np.iinfo(np.int32).min
BIG = ((-1e6, -1e6, -1e6), (1e6, 1e6, 1e6))
# x in [3, 6] beside the triangle, z in [-6, -4].  A camera ray reaches z = -6 at |x| <= 6 * 1.5 *
# tan(15 deg) = 2.41 < 3, so no camera ray enters it; a shadow ray towards LIGHT_PX starts at
# |x| <= 1, z = -5 and ends at x = 10, z = -4.5, so every one crosses it.
SIDE_BOX = ((3.0, -1e6, -6.0), (6.0, 1e6, -4.0))
LEFT_HALF = ((-1e6, -1e6, -1e6), (0.0, 1e6, 1e6))   # from the eye: exactly the rays with d.x < 0

TUNINGS = [dict(walk_exit=we, walk_latch=wl, scalar_nodes=sn) for we, wl, sn in itertools.product((0, 1), (0, 1), (0, 7))]
tuning_id = lambda k: "-".join(f"{a}{b}" for a, b in k.items())


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


def node(children, boxes):
    """One QBVH node for mrt_scene_bvh_import: four child words and the four slot boxes
    ((lo, hi) per slot) in the node's [lo x4 | lo y4 | lo z4 | hi x4 | hi y4 | hi z4] order."""
    b = np.zeros(24, np.float32)
    for i, (lo, hi) in enumerate(boxes):
        for a in range(3):
            b[4 * a + i] = lo[a]
            b[12 + 4 * a + i] = hi[a]
    return b, np.array(children, np.int32)


def leaf_node(box):
    return node([~0, EMPTY, EMPTY, EMPTY], [box] * 4)


def chain(depth, first=0, box=BIG, slot0_box=None, tail=None):
    """test_full_size.py's chain: `depth` nodes from index `first`, node k's slots 0-2 the leaf
    node L and its slot 3 (the highest, visited next) node k + 1 -- three entries pushed per
    node; the last node's slot 3 is `tail` (default L).  L follows the chain.  slot0_box: another
    box for every chain node's slot 0, so that only the rays inside it push a third entry."""
    L = first + depth
    out = []
    for k in range(depth):
        nxt = first + k + 1 if k + 1 < depth else (L if tail is None else tail)
        out.append(node([L, L, L, nxt], [slot0_box or box, box, box, box]))
    out.append(leaf_node(box))
    return out


def imported_scene(nodes, light):
    """The one-triangle scene with `nodes` in place of its built hierarchy."""
    cfg = dict(material=dict(kind="lambert", kd=(0.8, 0.8, 0.8)), bg=(0.1, 0.2, 0.3),
               lights=[dict(type="point", pos=light, power=100.0)], camera=CAM)
    P, _, _ = scene_pair(cfg, meshes=[TRI])
    _, _, lt, lp = P.bvh_export()
    nb = np.ascontiguousarray(np.stack([n[0] for n in nodes]))
    nc = np.ascontiguousarray(np.stack([n[1] for n in nodes]))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(miro.lib().mrt_scene_bvh_import(P.handle, len(nodes), len(lt), nb.ctypes.data_as(fp), nc.ctypes.data_as(ip),
                                               lt.ctypes.data_as(fp), lp.ctypes.data_as(ip)), "import")
    return P


@pytest.fixture(scope="module")
def refs():
    """The oracle's frame of the plain one-triangle scene per light position, computed once."""
    out = {}
    for light in (LIGHT, LIGHT_PX, LIGHT_NX):
        cfg = dict(material=dict(kind="lambert", kd=(0.8, 0.8, 0.8)), bg=(0.1, 0.2, 0.3),
                   lights=[dict(type="point", pos=light, power=100.0)], camera=CAM)
        _, Osc, cam = scene_pair(cfg, meshes=[TRI])
        ref = Osc.render(cam, W, H)
        prim = ref["hits"]["prim"]
        assert set(np.unique(prim)) == {-1, 0}, "the frame has covered and background pixels"
        tiles = [prim[y:y + 8, x:x + 8] for y in range(0, H, 8) for x in range(0, W, 8)]
        assert any((t >= 0).any() and (t < 0).any() for t in tiles), "a tile with both kinds of pixel"
        assert ref["shadow_rays"] == (prim == 0).sum(), "every hit casts its shadow ray"
        out[light] = ref
    return out


def assert_frame(P, ref):
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(CAM), img, want_hits=True)
    assert np.array_equal(hits["prim"], ref["hits"]["prim"]), "primary hit ids differ"
    hit = ref["hits"]["prim"] >= 0
    assert (hits["prim"][hit] == 0).all()
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(hits[k][hit]), bits(ref["hits"][k][hit])), f"hit {k} differs"
    # the closed form of test_full_size.py: every covered pixel's hit lies on z = -5 (the camera
    # looks down -z from the origin, so its ray's unit direction has d.z = -5 / t)
    assert np.all(hits["t"][hit] >= 5.0) and np.all(hits["t"][hit] < 5.0 * np.sqrt(1 + 0.41 ** 2 + 0.27 ** 2))
    assert np.array_equal(bits(img.rgb), bits(ref["rgb"])), "float RGB differs"
    assert np.array_equal(img.pixels, ref["rgb8"]), "8-bit RGB differs"
    assert P.last_stats["shadow_rays"] == ref["shadow_rays"]


_scenes = {}


def cached(key, build):
    if key not in _scenes:
        _scenes[key] = build()
    return _scenes[key]


# depth -> stack entries: 4 -> 12 and 5 -> 15 push four-entry blocks up to the boundary sp + 4 ==
# 16; 6 -> 18 crosses it (the first spill entries); 30 -> 90 into the HBM column; 85 -> 255, the
# reference's 256-entry stack nearly full; 86 -> 258: MRT_ERR_OVERFLOW
@pytest.mark.gpu
@pytest.mark.parametrize("knobs", TUNINGS, ids=tuning_id)
@pytest.mark.parametrize("depth", [4, 5, 6, 30, 85, 86])
def test_chain_depths_on_the_frame_kernel(refs, depth, knobs):
    need_gpu()
    P = cached(("chain", depth), lambda: imported_scene(chain(depth), LIGHT))
    with tuned(**knobs):
        if depth == 86:
            with pytest.raises(miro.MRTError, match="OVERFLOW"):
                assert_frame(P, refs[LIGHT])
        else:
            assert_frame(P, refs[LIGHT])


def side_chain(depth):
    """Root: slot 0 the triangle's leaf node (a box every ray crosses), slot 1 a chain of
    `depth` nodes in SIDE_BOX, which only shadow rays towards LIGHT_PX cross."""
    return [node([1, 2, EMPTY, EMPTY], [BIG, SIDE_BOX, BIG, BIG]), leaf_node(BIG)] + chain(depth, first=2, box=SIDE_BOX)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", TUNINGS, ids=tuning_id)
def test_overflow_from_the_shadow_walk_alone_and_the_frame_after_it(refs, knobs):
    """The deep chain lies beside the triangle.  Lit from the other side no ray meets it (the
    frame is exact: the camera rays' walk does not overflow); lit through it at depth 30 the
    shadow walk spills and the frame is exact; at depth 86 only the shadow walk overflows ->
    MRT_ERR_OVERFLOW; the next frame, of a shallow scene on the same stream, is OK and exact:
    the counter is not left set."""
    need_gpu()
    away = cached(("side", 86, "nx"), lambda: imported_scene(side_chain(86), LIGHT_NX))
    spill = cached(("side", 30, "px"), lambda: imported_scene(side_chain(30), LIGHT_PX))
    deep = cached(("side", 86, "px"), lambda: imported_scene(side_chain(86), LIGHT_PX))
    shallow = cached(("chain", 4), lambda: imported_scene(chain(4), LIGHT))
    with tuned(**knobs):
        assert_frame(away, refs[LIGHT_NX])
        assert_frame(spill, refs[LIGHT_PX])
        with pytest.raises(miro.MRTError, match="OVERFLOW"):
            assert_frame(deep, refs[LIGHT_PX])
        assert_frame(shallow, refs[LIGHT])


def mixed_chain():
    """A depth-5 chain whose nodes' slot 0 only the camera rays with d.x < 0 cross: those
    lanes push three entries per node (sp 15 after the chain), the others two (sp 10).  The
    chain ends in M, three leaf-node children: every lane pushes two more entries there --
    the left lanes from sp 15 (past the LDS column: entries 15 and 16), the right lanes from
    10.  The middle tiles straddle x = 0, so their waves hold both kinds of lane."""
    M, L = 5, 6
    nodes = chain(5, slot0_box=LEFT_HALF, tail=M)          # nodes 0-4, then its leaf node at index 5 ...
    nodes[5] = node([L, L, L, EMPTY], [BIG] * 4)           # ... which M replaces,
    for k in range(5):                                     # so the chain's leaf node moves to index 6
        nodes[k][1][:3] = L
    return nodes + [leaf_node(BIG)]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", TUNINGS, ids=tuning_id)
def test_tile_whose_lanes_disagree_on_the_rare_push(refs, knobs):
    """Some lanes of a wave push from sp >= 13 (entry by entry, into the spill column) in the
    step in which the others push their four-entry block: right whether the push block
    decides the rare case per lane or once per wave."""
    need_gpu()
    P = cached("mixed", lambda: imported_scene(mixed_chain(), LIGHT))
    with tuned(**knobs):
        img = miro.Image()
        img.resize(W, H)
        P.raytraceImage(camera(CAM), img, count_visits=True)
        assert P.last_stats["max_stack"] == 17, "the left lanes reach 15 + 2 entries"
        assert_frame(P, refs[LIGHT])


def test_walk_arrays_fit_limit():
    """Nodes are 128 B and leaf packets 160 B; each array must end within 4 GiB."""
    L = miro.lib()
    nodes, leaves = 2 ** 32 // 128, 2 ** 32 // 160
    assert nodes * 128 == 2 ** 32 and leaves * 160 <= 2 ** 32 < (leaves + 1) * 160
    assert L.mrt_walk_arrays_fit(0, 0) == 1
    assert L.mrt_walk_arrays_fit(9084, 18162) == 1          # the Sponza stand-in
    assert L.mrt_walk_arrays_fit(nodes, leaves) == 1
    assert L.mrt_walk_arrays_fit(nodes + 1, leaves) == 0
    assert L.mrt_walk_arrays_fit(nodes, leaves + 1) == 0
    assert L.mrt_walk_arrays_fit(nodes + 1, 0) == 0 and L.mrt_walk_arrays_fit(0, leaves + 1) == 0
    assert L.mrt_walk_arrays_fit(2 ** 63, 1) == 0 and L.mrt_walk_arrays_fit(1, 2 ** 63) == 0   # no wrap-around
