"""The walk loops of traverse_impl (csrc/mrt_kernels.h) on the frame kernel: the closest
hit read from the hit record (packed slot 0 is a hit), the scalar node fetch through the
wave's octant rows, and every walk tuning, each frame bit for bit against the CPU oracle:
float and 8-bit RGB, the hit records, the shadow-ray count and the primary node and leaf
visits; a render without hit records gives the same pixels as one with them."""
import numpy as np
import pytest

import miro
from helpers import bits, camera, fixture_mesh, scene_pair, tuned
from miro import scenes

pytestmark = pytest.mark.gpu

LAMBERT = dict(kind="lambert", kd=(0.8, 0.8, 0.8))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


def render(P, cam, W, H, **kw):
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(cam), img, **kw)
    return img, hits


def assert_frame(P, cam, W, H, ref):
    """One frame of P with hit records and visit counts against the oracle's `ref`, then the
    same frame without hit records."""
    img, hits = render(P, cam, W, H, want_hits=True, count_visits=True)
    assert np.array_equal(bits(img.rgb), bits(ref["rgb"])), "float RGB differs"
    assert np.array_equal(img.pixels, ref["rgb8"]), "8-bit RGB differs"
    assert np.array_equal(hits["prim"], ref["hits"]["prim"]), "primary hit ids differ"
    hit = ref["hits"]["prim"] >= 0
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(hits[k][hit]), bits(ref["hits"][k][hit])), f"hit {k} differs"
    st = P.last_stats
    assert st["shadow_rays"] == ref["shadow_rays"]
    assert st["primary_node_visits"] == ref["primary_node_visits"]
    assert st["primary_leaf_visits"] == ref["primary_leaf_visits"]
    img2, none = render(P, cam, W, H)
    assert none is None
    assert np.array_equal(bits(img2.rgb), bits(ref["rgb"])), "float RGB differs without hit records"
    assert np.array_equal(img2.pixels, ref["rgb8"]), "8-bit RGB differs without hit records"


def test_single_triangle_packed_slot_zero_is_a_hit():
    """One triangle: its leaf is leaf 0 and it is lane 0 there, so every covered pixel's
    packed slot (leaf << 2 | lane) is 0 -- a hit, told from a miss (-1) by prim >= 0."""
    verts = np.array([(-1.0, -0.8, 0.0), (1.2, -0.6, 0.0), (0.1, 0.9, 0.0)], np.float32)
    normals = np.array([(0.0, 0.0, 1.0)], np.float32)
    mesh = (verts, normals, np.array([(0, 1, 2)], np.uint32), np.array([(0, 0, 0)], np.uint32))
    cfg = dict(material=LAMBERT, bg=(0.1, 0.2, 0.3), lights=[dict(type="point", pos=(0.5, 0.6, 2.0), power=30.0)],
               camera=dict(eye=(0.0, 0.0, 3.0), lookAt=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=45.0))
    P, Osc, cam = scene_pair(cfg, meshes=[mesh])
    W, H = 40, 24
    ref = Osc.render(cam, W, H)
    prim = ref["hits"]["prim"]
    assert set(np.unique(prim)) == {-1, 0}, "some pixels hit the triangle and some miss it"
    bg = np.broadcast_to(np.float32(cfg["bg"]), ref["rgb"].shape)
    assert np.array_equal(bits(ref["rgb"])[prim < 0], bits(bg)[prim < 0])
    assert (bits(ref["rgb"])[prim == 0] != bits(bg)[prim == 0]).any(axis=-1).all(), "a lit hit is not the background"
    assert_frame(P, cam, W, H, ref)


# cornell_box from its centre: eight diagonal views (the whole frame inside one direction-sign
# octant: the frame's corner is 29 degrees off the axis, the octant's nearest face 35) and three
# axis-aligned ones (the centre tiles straddle two sign changes)
CENTRE = (2.75, 2.75, -2.75)
DIAGONALS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
VIEWS = [dict(eye=CENTRE, lookAt=tuple(c + s for c, s in zip(CENTRE, d)), up=(0, 1, 0), fov=30.0) for d in DIAGONALS] + [
    dict(eye=CENTRE, lookAt=(2.75, 2.75, -5.0), up=(0, 1, 0), fov=55.0),
    dict(eye=CENTRE, lookAt=(5.0, 2.75, -2.75), up=(0, 1, 0), fov=55.0),
    dict(eye=CENTRE, lookAt=(2.75, 0.5, -2.75), up=(0, 0, -1), fov=55.0)]


def tile_octants(cam, W, H):
    """Per 8x8 tile (one wave of the frame kernel) the set of direction-sign octants of its
    pixels' camera rays: the pinhole ray of Camera::eyeRayAdaptive through the pixel centre."""
    eye, look, up = (np.array(cam[k], np.float64) for k in ("eye", "lookAt", "up"))
    unit = lambda v: v / np.linalg.norm(v)
    w = -unit(look - eye)
    u = unit(np.cross(unit(up), w))
    v = np.cross(w, u)
    top = np.tan(np.radians(cam["fov"]) / 2)
    right = top * W / H
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    Up = -right + 2 * right * (x + 0.5) / W
    Vp = -top + 2 * top * (y + 0.5) / H
    d = Up[..., None] * u + Vp[..., None] * v - w
    assert np.abs(d).min() > 1e-6, "no ray sits on an octant boundary"
    oct_ = (d[..., 0] < 0) * 1 + (d[..., 1] < 0) * 2 + (d[..., 2] < 0) * 4
    return [set(np.unique(oct_[ty:ty + 8, tx:tx + 8])) for ty in range(0, H, 8) for tx in range(0, W, 8)]


@pytest.fixture(scope="module")
def cornell():
    cfg = dict(scenes.CONFIGS["C1"], material=LAMBERT)
    P, Osc, _ = scene_pair(cfg, meshes=[fixture_mesh("cornell_box")])
    return P, Osc


def test_views_cover_every_octant_and_a_mixed_tile():
    tiles = [t for cam in VIEWS for t in tile_octants(cam, 72, 40)]
    uniform = set().union(*[t for t in tiles if len(t) == 1])
    assert uniform == set(range(8)), uniform
    assert any(len(t) > 1 for t in tiles)
    for cam in VIEWS[:8]:
        assert all(len(t) == 1 for t in tile_octants(cam, 72, 40))
    for cam in VIEWS[8:]:
        assert any(len(t) > 1 for t in tile_octants(cam, 72, 40))


@pytest.mark.parametrize("view", range(len(VIEWS)))
def test_cornell_octant_views_match_oracle(cornell, view):
    """72 x 40: partly empty 8x8 tiles at the right edge; one view per octant, then the mixed ones."""
    P, Osc = cornell
    cam = VIEWS[view]
    ref = Osc.render(cam, 72, 40)
    assert (ref["hits"]["prim"] >= 0).any()
    assert_frame(P, cam, 72, 40, ref)


# explosion01 (11,647 nodes, leaves of 1-4 triangles, 2- and 3-child nodes) seen from the front,
# lit from the side at a low angle, so its relief blocks part of the shadow rays
EXPLOSION = dict(material=LAMBERT, bg=(0.1, 0.2, 0.3), lights=[dict(type="point", pos=(0.9, 0.9, 0.25), power=20.0)],
                 camera=dict(eye=(0.0, 0.5, 1.6), lookAt=(0.0, 0.5, 0.05), up=(0, 1, 0), fov=40.0))


@pytest.fixture(scope="module")
def explosion():
    P, Osc, cam = scene_pair(EXPLOSION, meshes=[fixture_mesh("explosion01")])
    ref = Osc.render(cam, 96, 64, threads=8)
    return P, cam, ref


def test_explosion_reference_has_blocked_and_free_shadow_rays(explosion):
    _, _, ref = explosion
    assert (ref["hits"]["prim"] >= 0).mean() > 0.3
    occluded = (ref["shadow"] > 0).sum() / ref["shadow_rays"]
    assert 0.1 < occluded < 0.9, occluded


@pytest.mark.parametrize("knobs", [dict(walk_latch=0), dict(walk_latch=1), dict(walk_exit=0), dict(walk_exit=1),
                                   dict(scalar_nodes=0), dict(scalar_nodes=3), dict(scalar_nodes=7),
                                   dict(lds_nodes=1)], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_explosion_matches_oracle_under_walk_tunings(explosion, knobs):
    P, cam, ref = explosion
    with tuned(**knobs):
        assert_frame(P, cam, 96, 64, ref)
        if knobs.get("lds_nodes"):   # the hierarchy has the 64 nodes the LDS top-node walk stages
            assert P.walk_info()["lds_nodes"] == 1
