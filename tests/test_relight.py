"""Relighting in place (mrt_scene_update_lights / _material / _texture and their async forms;
miro.Scene.updateLights / updateMaterial / updateTexture): after an update a scene is, bit for
bit, the scene built fresh with the new values -- frames, hit records, shadow-ray counts,
sampleLights, lightSamples and, for a dome light's texture, every table DomeLight::setTexture
makes (the device builds them: csrc/mrt_relight.hip) -- and it was not uploaded again.

Every comparison is on float bits; two NaNs count as equal (a black column's normalised CDF is
0/0 and x/0: the host's NaN and the device's differ in sign).  Frames are 37 x 29.

Resources: the first texture update of a replica allocates its scratch, so
mrt_debug_live_resources is compared across the updates that follow it, and across every light
and material update, which allocate nothing; the upload count is compared across everything."""
import ctypes as C

import numpy as np
import pytest

import miro
from helpers import bits, camera, fixture_mesh, scene_pair
from miro import _lib, scenes
from test_ibl import dome_oracle
from test_sample_rays import BLINN, CAM, POINT, RECT

W, H = 37, 29
FAR = dict(CAM, eye=(2.75, 2.75, 16.0))   # dome_scene()'s camera: rays pass the box and miss
INVALID = -1


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


def last_error():
    return miro.lib().mrt_last_error().decode()


def same(a, b):
    """Equal bits, or NaN in both."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------ skies and scenes
def sky(w, h, seed, black=False):
    """A seeded positive sky (h, w, 3); black: one all-black column and one all-black row."""
    rgb = np.random.default_rng(seed).uniform(0.05, 4.0, (h, w, 3)).astype(np.float32)
    if black:
        rgb[:, w // 3] = 0
        rgb[h // 2, :] = 0
    return rgb


def dome_scene(rgb, power=0.15, samples=3, lights=None, **kw):
    """tests/test_sample_rays.py dome_scene() with the sky given as texels: one texture that
    is the environment map and the dome light's."""
    cfg = dict(scenes.CONFIGS["C1"], material=BLINN, env=dict(sky=rgb, exposure=1.5),
               lights=[dict(type="dome", sky=rgb, power=power, samples=samples, noise=0.001)] + list(lights or []))
    return scene_pair(cfg, meshes=[fixture_mesh("cornell_box")], **kw)[0]


def cornell(material, lights, **kw):
    cfg = dict(scenes.CONFIGS["C1"], material=material)
    return scene_pair(cfg, meshes=[fixture_mesh("cornell_box")], lights=lights, **kw)[0]


def probe_points(n=257, seed=4):
    """Points inside the Cornell box with unit normals (more than one workgroup of them)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.6, 4.9, (n, 3)).astype(np.float32)
    p[:, 2] = -p[:, 2]
    d = rng.normal(size=(n, 3))
    return p, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def dome_state(P, light=0):
    return dict(P.dome_tables(light), **P.domeTablesDerived(light))


def state(P, cam=CAM, seed=7, dome=None, samples=True):
    """Everything a caller can see of the lighting: a frame with its hit records and shadow-ray
    count, sampleLights and lightSamples at the probe points, the tables of dome light `dome`."""
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(cam), img, want_hits=True, seed=seed)
    out = dict(rgb=img.rgb.copy(), **{k: np.int64(P.last_stats[k]) for k in ("shadow_rays", "fused", "chain")})
    for k in ("t", "a", "b", "prim", "inst"):
        out["hit_" + k] = hits[k].copy()
    p, n = probe_points()
    e, per = P.sampleLights(p, n, seed=seed, per_light=True)
    out.update(e=e, per=per)
    if samples:
        ls = P.lightSamples(p, n, seed=seed)
        out.update(ls_samples=np.ascontiguousarray(ls["samples"]).view(np.uint8), ls_counts=ls["counts"])
    if dome is not None:
        out.update(dome_state(P, dome))
    return out


def assert_same_state(got, want):
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not same(got[k], want[k])]
    assert not bad, bad


def live():
    return miro.lib().mrt_debug_live_resources()


def dome_texture(P, light=0):
    return P._lights[light].texture


def torch_stream():
    import torch
    return torch, torch.cuda.Stream(device=0)


def update_texture_async(P, tex, rgb):
    """updateTexture with a device tensor on a side stream; returns after the stream is idle."""
    torch, st = torch_stream()
    t = torch.from_numpy(rgb).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert P.updateTexture(tex, t, stream=st) is None
    st.synchronize()


# ------------------------------------------------------------------ CPU: the ABI
NEW = ["mrt_scene_update_lights", "mrt_scene_update_lights_async", "mrt_scene_update_material",
       "mrt_scene_update_material_async", "mrt_scene_update_texture", "mrt_scene_update_texture_async",
       "mrt_scene_texture_update_status", "mrt_scene_dome_export_derived", "mrt_scene_upload_count"]


def test_the_nine_symbols_are_exported_and_wrapped():
    L = miro.lib()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.mrt_abi_version() == 10
    for name in ("updateLights", "updateMaterial", "updateTexture", "textureUpdateStatus", "domeTablesDerived", "uploadCount"):
        assert callable(getattr(miro.Scene, name))


def small_scene():
    """A built dome scene that is never uploaded (no device call may happen on it)."""
    return dome_scene(sky(16, 8, 1), lights=[RECT, POINT])


def light_array(P):
    return (_lib.mrt_light * len(P._lights))(*[P._light_c(l) for l in P._lights])


def test_every_refusal_comes_before_a_device_call_with_its_own_text():
    L = miro.lib()
    P = small_scene()
    h, arr = P.handle, light_array(P)
    m = list(P._mat_objs.values())[0]._c()
    tex = np.zeros((8, 16, 3), np.float32)
    ms = C.c_float(0)
    seen = []

    def refused(rc, *words):
        assert rc == INVALID
        err = last_error()
        for w in words:
            assert w in err, (w, err)
        seen.append(err)

    for f, args in ((L.mrt_scene_update_lights, (arr, 3)), (L.mrt_scene_update_lights_async, (arr, 3, None))):
        refused(f(None, *args), "null scene")
        refused(f(h, None, *args[1:]), "null lights")
        refused(f(h, arr, 2, *args[2:]), "2 lights given", "the scene has 3")
    for f, tail in ((L.mrt_scene_update_material, ()), (L.mrt_scene_update_material_async, (None,))):
        refused(f(None, 0, C.byref(m), *tail), "null scene")
        refused(f(h, 0, None, *tail), "null material")
        refused(f(h, 99, C.byref(m), *tail), "bad material id 99")
        refused(f(h, -1, C.byref(m), *tail), "bad material id -1")
        lam = miro.Lambert()._c()
        refused(f(h, 0, C.byref(lam), *tail), "material 0 changes its type")
    for f, tail in ((L.mrt_scene_update_texture, (C.byref(ms),)), (L.mrt_scene_update_texture_async, (None,))):
        refused(f(None, 0, tex.ctypes.data, *tail), "null scene")
        refused(f(h, 0, None, *tail), "null texels")
        refused(f(h, 7, tex.ctypes.data, *tail), "bad texture id 7")
        refused(f(h, -1, tex.ctypes.data, *tail), "bad texture id -1")
    n = C.c_int32(5)
    refused(L.mrt_scene_texture_update_status(None, C.byref(n)), "null argument")
    refused(L.mrt_scene_texture_update_status(h, None), "null argument")
    refused(L.mrt_scene_dome_export_derived(h, 1, None, None, None), "not a dome light")
    assert L.mrt_scene_upload_count(None) == INVALID
    # each light keeps its type, its texture and its transparent_shadows; the light and the field are named
    for i, field, value in ((1, "type", 0), (0, "texture", 5), (2, "transparent_shadows", 1), (1, "transparent_shadows", 1)):
        arr = light_array(P)
        setattr(arr[i], field, value)
        refused(L.mrt_scene_update_lights(h, arr, 3), f"light {i} changes its {field}")
        refused(L.mrt_scene_update_lights_async(h, arr, 3, None), f"light {i} changes its {field}")
    # the async forms on a scene that is not uploaded
    refused(L.mrt_scene_update_lights_async(h, light_array(P), 3, None), "exactly one device")
    refused(L.mrt_scene_update_material_async(h, 0, C.byref(m), None), "exactly one device")
    refused(L.mrt_scene_update_texture_async(h, 0, tex.ctypes.data, None), "exactly one device")
    assert len(set(seen)) >= 14
    assert P.uploadCount() == 0 and P.textureUpdateStatus() == 0


def test_the_wrapper_refuses_wrong_shapes_and_dtypes():
    P = small_scene()
    tex = dome_texture(P)
    for bad in (np.zeros((8, 16), np.float32), np.zeros((16, 8, 3), np.float32), np.zeros((8, 16, 4), np.float32),
                np.zeros((8, 16, 3), np.float64)):
        with pytest.raises(miro.MRTError, match="updateTexture"):
            P.updateTexture(tex, bad)
    with pytest.raises(miro.MRTError, match="not a texture of this scene"):
        P.updateTexture(miro.Texture(miro.RawImage(16, 8, np.zeros((8, 16, 3), np.float32))), np.zeros((8, 16, 3), np.float32))
    with pytest.raises(miro.MRTError, match="not a material of this scene"):
        P.updateMaterial(miro.Lambert())
    assert P.uploadCount() == 0


# ------------------------------------------------------------------ CPU: a built scene that is not uploaded
@pytest.mark.parametrize("w,h,black", [(16, 8, False), (70, 33, True), (1, 1, False)])
def test_host_texture_update_equals_a_fresh_scene_and_the_oracle(w, h, black):
    new = sky(w, h, 2, black)
    P = dome_scene(sky(w, h, 1))
    assert P.updateTexture(dome_texture(P), new) == 0.0
    got, fresh, orc = dome_state(P), dome_state(dome_scene(new)), dome_oracle(new)
    assert sorted(got) == sorted(fresh)
    assert not [k for k in fresh if not same(got[k], fresh[k])]
    assert not [k for k in orc if not same(got[k], orc[k])]
    assert P.uploadCount() == 0


def test_host_texture_update_refuses_a_black_sky_and_keeps_the_old_one():
    P = dome_scene(sky(16, 8, 1))
    before = dome_state(P)
    with pytest.raises(miro.MRTError, match="no positive radiance"):
        P.updateTexture(dome_texture(P), np.zeros((8, 16, 3), np.float32))
    after = dome_state(P)
    assert not [k for k in before if not same(after[k], before[k])]
    # the old texels are back: building the tables again from them gives the old tables
    assert P.updateTexture(dome_texture(P), sky(16, 8, 1)) == 0.0
    assert not [k for k in before if not same(dome_state(P)[k], before[k])]


def test_host_light_update_makes_the_records_a_fresh_add_light_makes():
    """On the host the DevLight records are visible through a re-upload only, so this compares
    what mrt_scene_update_lights accepts and keeps: after new vertices and power on the
    rectangle light, a second update with the very same values is accepted (type, texture and
    transparent_shadows are compared against the stored arguments), and the dome's tables are
    untouched.  The GPU test compares the records themselves, through sampleLights."""
    P = small_scene()
    before = dome_state(P)
    rect = P._lights[1]
    rect.setVertices((1.0, 5.4, -1.0), (1.0, 5.4, -2.5), (3.0, 5.4, -1.0))
    rect.setPower(40.0)
    rect.setSamples(0)   # clamped to 1 by the conversion
    P.updateLights()
    P.updateLights()
    assert not [k for k in before if not same(dome_state(P)[k], before[k])]
    assert P.uploadCount() == 0


# ------------------------------------------------------------------ GPU: texture updates
SIZES = [(64, 32), (70, 33), (130, 67), (257, 5), (1, 1)]   # the fixture's; no multiple of 64 / 32; three column tiles with a
                                                           # partial one; fewer rows than a tile; the smallest build_dome takes
PATTERNS = [(w, h, black) for w, h in SIZES for black in (False, True) if not (black and (w, h) == (1, 1))]
_fresh = {}


def fresh_dome(w, h, seed, black):
    """The state of a scene built with sky(w, h, seed, black), computed once."""
    key = (w, h, seed, black)
    if key not in _fresh:
        _fresh[key] = state(dome_scene(sky(w, h, seed, black)), FAR, dome=0)
    return _fresh[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("w,h,black", PATTERNS)
def test_a_texture_update_equals_a_fresh_scene(w, h, black, form):
    need_gpu()
    new = sky(w, h, 2, black)
    P = dome_scene(sky(w, h, 1))
    state(P, FAR, samples=False)   # uploaded, one frame rendered with the old sky
    n_up = P.uploadCount()
    if form == "sync":
        assert P.updateTexture(dome_texture(P), new) >= 0.0
    else:
        update_texture_async(P, dome_texture(P), new)
        assert P.textureUpdateStatus() == 0
    assert_same_state(state(P, FAR, dome=0), fresh_dome(w, h, 2, black))
    assert P.uploadCount() == n_up == 1


@pytest.mark.gpu
def test_a_black_sky_is_rejected_by_both_forms_and_changes_nothing():
    need_gpu()
    w, h = 70, 33
    P = dome_scene(sky(w, h, 1))
    old = state(P, FAR, dome=0)
    black = np.zeros((h, w, 3), np.float32)
    with pytest.raises(miro.MRTError, match="no positive radiance"):
        P.updateTexture(dome_texture(P), black)
    assert_same_state(state(P, FAR, dome=0), old)
    assert P.textureUpdateStatus() == 0   # a synchronous refusal is returned, not counted
    update_texture_async(P, dome_texture(P), black)
    assert P.textureUpdateStatus() == 1
    assert P.textureUpdateStatus() == 0
    assert_same_state(state(P, FAR, dome=0), old)
    # a good update after the refused ones, either form
    update_texture_async(P, dome_texture(P), sky(w, h, 2, True))
    assert P.textureUpdateStatus() == 0
    assert_same_state(state(P, FAR, dome=0), fresh_dome(w, h, 2, True))
    P.updateTexture(dome_texture(P), sky(w, h, 2))
    assert_same_state(state(P, FAR, dome=0), fresh_dome(w, h, 2, False))
    assert P.uploadCount() == 1


@pytest.mark.gpu
def test_two_updates_in_a_row_leave_the_second_sky_and_allocate_nothing_more():
    need_gpu()
    w, h = 130, 67
    P = dome_scene(sky(w, h, 1))
    state(P, FAR, samples=False)
    P.updateTexture(dome_texture(P), sky(w, h, 3, True))   # (the first update allocates the scratch)
    update_texture_async(P, dome_texture(P), sky(w, h, 3, True))
    held = live()
    P.updateTexture(dome_texture(P), sky(w, h, 2))
    update_texture_async(P, dome_texture(P), sky(w, h, 2, True))
    assert live() == held
    assert_same_state(state(P, FAR, dome=0), fresh_dome(w, h, 2, True))
    assert P.uploadCount() == 1


@pytest.mark.gpu
def test_the_environment_map_texture_alone():
    """A texture that feeds no dome light: the update is a copy, and the miss pixels follow."""
    need_gpu()
    def build(rgb):
        cfg = dict(scenes.CONFIGS["C1"], material=BLINN, env=dict(sky=rgb, exposure=1.5))
        return scene_pair(cfg, meshes=[fixture_mesh("cornell_box")], lights=[POINT])[0]
    old, new = sky(40, 20, 1), sky(40, 20, 2)
    want = state(build(new), FAR)
    assert (want["hit_prim"] < 0).any()
    for form in ("sync", "async"):
        P = build(old)
        first = state(P, FAR)
        assert not same(first["rgb"], want["rgb"])
        if form == "sync":
            P.updateTexture(P.m_envMap, new)
        else:
            update_texture_async(P, P.m_envMap, new)
        assert_same_state(state(P, FAR), want)
        assert P.uploadCount() == 1


@pytest.mark.gpu
def test_the_colour_map_of_the_leaves_scene():
    need_gpu()
    from test_textures import leaf_image, leaves_scene

    def colour_map(P):
        return [m.colorMap for m in P._mat_objs.values() if getattr(m, "colorMap", None) is not None][0]
    img, typ = leaf_image()
    new = img.copy()
    new[..., :3] = new[..., :3][..., ::-1] * np.float32(0.5)
    P = leaves_scene(alpha=False)[0]
    first = state(P)
    assert P.updateTexture(colour_map(P), new) >= 0.0
    got = state(P)
    # the fresh scene: the same build with the new image as its colour map
    import test_textures
    saved = test_textures.leaf_image
    test_textures.leaf_image = lambda: (new, typ)
    try:
        want = state(leaves_scene(alpha=False)[0])
    finally:
        test_textures.leaf_image = saved
    assert not same(first["rgb"], want["rgb"])
    assert_same_state(got, want)
    assert P.uploadCount() == 1


# ------------------------------------------------------------------ GPU: lights
RECT2 = dict(RECT, v1=(1.0, 5.4, -1.0), v2=(1.0, 5.4, -2.5), v3=(3.0, 5.4, -1.0), power=31.0, samples=5, noise=0.01)
POINT2 = dict(POINT, pos=(1.5, 4.0, -1.0), power=33.0)


def relight(P, form):
    if form == "sync":
        P.updateLights()
    else:
        torch, st = torch_stream()
        torch.cuda.synchronize()
        P.updateLights(stream=st)
        st.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sync", "async"])
def test_light_updates_equal_a_fresh_scene(form):
    """The point light moves, the rectangle light gets new vertices, power, samples and noise
    (its area scaling changes), the dome its gain and samples."""
    need_gpu()
    rgb = sky(64, 32, 1)
    want = state(dome_scene(rgb, power=0.4, samples=2, lights=[RECT2, POINT2], num_paths=2), FAR, dome=0)
    P = dome_scene(rgb, lights=[RECT, POINT], num_paths=2)
    first = state(P, FAR, dome=0)
    assert not same(first["e"], want["e"]) and not same(first["rgb"], want["rgb"])
    dome, rect, point = P._lights
    point.setPosition(POINT2["pos"]); point.setPower(POINT2["power"])
    rect.setVertices(RECT2["v1"], RECT2["v2"], RECT2["v3"]); rect.setPower(RECT2["power"])
    rect.setSamples(RECT2["samples"]); rect.setNoiseThreshold(RECT2["noise"])
    dome.setPower(0.4); dome.setSamples(2)
    held = live()
    relight(P, form)
    assert live() == held
    assert_same_state(state(P, FAR, dome=0), want)
    assert P.uploadCount() == 1


@pytest.mark.gpu
def test_a_moved_point_light_on_the_one_light_and_the_path_traced_scenes():
    need_gpu()
    for kw in (dict(), dict(path_trace=(3, False), num_paths=2)):
        mat = dict(kind="blinn", kd=(0.7, 0.6, 0.5))
        want = state(cornell(mat, [POINT2], **kw))
        P = cornell(mat, [POINT], **kw)
        assert not same(state(P)["rgb"], want["rgb"])
        P._lights[0].setPosition(POINT2["pos"]); P._lights[0].setPower(POINT2["power"])
        held = live()
        P.updateLights()
        assert live() == held
        got = state(P)
        assert_same_state(got, want)
        assert got["chain"] == (1 if kw else 0)
        assert P.uploadCount() == 1


# ------------------------------------------------------------------ GPU: materials
def walls(P):
    return list(P._mat_objs.values())[0]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sync", "async"])
def test_kd_and_ks_equal_a_fresh_scene(form):
    need_gpu()
    a = dict(kind="blinn", kd=(0.8, 0.5, 0.25), specExp=10.0, specAmt=0.4)
    P, F = cornell(a, [RECT, POINT]), cornell(a, [RECT, POINT])
    # the fresh scene: built (preCalc makes a new scene from the objects) with the new values from the start
    walls(F).setKd((0.2, 0.9, 0.4)); walls(F).setKs((0.5, 0.6, 0.7))
    F.preCalc()
    want = state(F)
    assert not same(state(P)["rgb"], want["rgb"])
    walls(P).setKd((0.2, 0.9, 0.4)); walls(P).setKs((0.5, 0.6, 0.7))
    held = live()
    if form == "sync":
        P.updateMaterial(walls(P))
    else:
        torch, st = torch_stream()
        torch.cuda.synchronize()
        P.updateMaterial(walls(P), stream=st)
        st.synchronize()
    assert live() == held
    assert_same_state(state(P), want)
    assert P.uploadCount() == 1


@pytest.mark.gpu
def test_spec_exp_from_1_to_8_and_back_moves_between_the_pow_free_and_the_pow_kernels():
    """One point light, Blinn walls: frame1_kernel's POW variant is picked by ImageInfo::pow_spec,
    which the update recomputes on the replica."""
    need_gpu()
    def mat(e):
        return dict(kind="blinn", kd=(0.8, 0.5, 0.25), specExp=e, specAmt=0.4)
    want1, want8 = state(cornell(mat(1.0), [POINT])), state(cornell(mat(8.0), [POINT]))
    assert not same(want1["rgb"], want8["rgb"])
    P = cornell(mat(1.0), [POINT])
    assert_same_state(state(P), want1)
    assert want1["fused"] == 1 and want8["fused"] == 1
    for e, want in ((8.0, want8), (1.0, want1), (8.0, want8)):
        walls(P).setSpecExp(e)
        held = live()
        P.updateMaterial(walls(P))
        assert live() == held
        assert_same_state(state(P), want)
    assert P.uploadCount() == 1


@pytest.mark.gpu
def test_emission_on_the_path_traced_scene():
    need_gpu()
    from test_path_trace import panel
    def build(emitted, le):
        return cornell(dict(kind="blinn", kd=(0.7, 0.7, 0.7)), [POINT], path_trace=(3, False), num_paths=2,
                       extra=[(panel(), dict(kind="blinn", kd=(1, 1, 1), emitted=emitted, le=le))])
    want = state(build(2.5, (1.0, 0.8, 0.6)))
    P = build(0.0, (0, 0, 0))
    assert not same(state(P)["rgb"], want["rgb"])
    pm = list(P._mat_objs.values())[1]
    pm.setLightEmittedIntensity(2.5); pm.setLightEmittedColor((1.0, 0.8, 0.6))
    P.updateMaterial(pm)
    assert_same_state(state(P), want)
    assert P.uploadCount() == 1


# ------------------------------------------------------------------ GPU: uploads and the host copy
@pytest.mark.gpu
def test_an_old_setter_uploads_again_and_the_host_copy_it_reads_is_the_devices():
    """After an async texture update the host copy is stale; dome_export reads it back, and a
    re-upload (forced here by an old setter) is made from what the device held."""
    need_gpu()
    w, h = 70, 33
    P = dome_scene(sky(w, h, 1))
    state(P, FAR, samples=False)
    update_texture_async(P, dome_texture(P), sky(w, h, 2, True))
    want = fresh_dome(w, h, 2, True)
    got = dome_state(P)   # sync_host
    assert not [k for k in got if not same(got[k], want[k])]
    update_texture_async(P, dome_texture(P), sky(w, h, 2))   # stale again: texels and tables
    assert P.uploadCount() == 1
    _lib.check(miro.lib().mrt_scene_set_material_sample_env(P.handle, 0, 1), "sample_env")   # marks the scene dirty
    assert_same_state(state(P, FAR, dome=0), fresh_dome(w, h, 2, False))
    assert P.uploadCount() == 2
    # and an update on the new replica works as on the first
    P.updateTexture(dome_texture(P), sky(w, h, 2, True))
    assert_same_state(state(P, FAR, dome=0), want)
    assert P.uploadCount() == 2
