"""The oracle against the reference renderer's own code.

Every other parity test here ends at oracle/, a restatement of the reference written by the
hands that wrote the kernels.  These tests compare that restatement with the reference itself,
compiled from its sources by oracle/ref/Makefile into oracle/_ref/ref_driver and driven through
oracle/refdriver.py on the cases of tests/reference_cases.py:

  exact tier        uint32 bits (oracle under LIBM_FLOAT, conftest's default): the OBJ loader, the
                    tree and its traversal (hit records and per-ray node / leaf visit counts: the
                    reference's BVH::rayBoxIntersections and Ray::rayTriangleIntersections count
                    the events the oracle's node_visits and leaf_visits count, one per node
                    popped and one per leaf packet tested, nested instance trees included, so
                    equal counts on every ray pin the tree and the order it is walked in),
                    deterministic shading, and stochastic shading with the oracle's draws
                    replayed through the reference's random-number pool;
  deep tier         uint32 bits at every chain level, path and eye ray: the oracle logs the key of
                    every draw it takes, in call order; the driver lays oro_rand of those keys into
                    the reference's pool, NaN after them, and runs the whole of
                    Scene::adaptiveSampleScene.  Frames, 8-bit pixels and the number of draws the
                    reference consumed per pixel must all be the oracle's.  Also the two gamma
                    tables, Map() and RawImage's decoders;
  statistical tier  the oracle's frame against the reference's distribution over 64 replicas:
                    what a single replayed frame cannot show (behaviour across many paths).

Two halves.  The live half needs the driver and skips without it (only where the reference's
sources exist must the driver exist: test_driver_built_where_reference_exists).  The recorded
half needs nothing but tests/golden/reference/ (written from the driver by
oracle/ref/make_reference_fixtures.py) and checks that the oracle reproduces every recorded
output; tests/test_reference_gpu.py holds the device to the same files.

The cases keep clear of two places where the reference reads memory it never wrote, and
Blinn's roulette reads its draw even for amounts of exactly 0 and 1, so those cases are in
the replayed tier ("Pinned to the reference").

The oracle has no any-hit entry point.  The shadow-query half of the traversal tests therefore
compares the reference's IS_SHADOW_RAY results with the oracle's closest-hit trace (same hit
flag, same t: the reference's shadow rays walk to the closest hit too); the oracle's own shadow
walk (trace_shadow, transmit) is pinned through the frames only.
"""
import numpy as np
import pytest

import oracle as O
import refdriver
import reference_cases as RC
from helpers import bits

live = pytest.mark.skipif(not refdriver.available(), reason="oracle/_ref/ref_driver is not built (no reference sources here)")

DET = RC.deterministic_cases()
REPLAY = RC.replay_cases()
STAT = RC.statistical_cases()
DEEP = RC.deep_cases()


def test_driver_built_where_reference_exists():
    if refdriver.reference_present():
        assert refdriver.available(), "the reference's sources are here but oracle/_ref/ref_driver is not: " \
                                      "make -C oracle/ref failed (build() prints its output)"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(
        a.view(np.uint32) if a.dtype.kind == "f" else a, b.view(np.uint32) if b.dtype.kind == "f" else b)


# ------------------------------------------------------------------ loader
@live
@pytest.mark.parametrize("model", RC.LOADER_MODELS)
def test_loader_matches_the_reference(model):
    ours = RC.oracle_loader_arrays(model)
    theirs = RC.reference_loader_arrays(model)      # array lengths counted by the driver from the file
    assert sorted(ours) == sorted(theirs)
    for k in ours:
        assert same_bits(ours[k], theirs[k]), k


@pytest.mark.parametrize("model", RC.LOADER_MODELS)
def test_loader_matches_the_recorded_reference(model):
    ours, rec = RC.oracle_loader_arrays(model), RC.fixture_json()["loader"][model]
    assert sorted(ours) == sorted(rec)
    for k in ours:
        assert list(ours[k].shape) == rec[k]["shape"] and RC.sha(ours[k]) == rec[k]["sha256"], k
    if model in ("Final/flower01Petals.obj", "sphere2.obj"):   # texture coordinates and shared normals
        assert "tangents" in ours and np.bincount(ours["nidx"].ravel()).max() > 1
        assert RC.written_tangent_slots(ours).all() and np.abs(ours["tangents"]).sum(1).min() > 0
    if model == "Final/cannonBallT1.obj":       # some triangles' uv edges are parallel: not every slot is written
        assert (ours["uv"].size and not RC.written_tangent_slots(ours).all())


# ------------------------------------------------------------------ tree and traversal
def check_trace(Os, o, d, tmin, tmax, ref):
    """ref: dict of hit, t, a, b, prim, nodes, leaves, shadow_hit, shadow_t for these rays."""
    h, nv, lv = Os.trace(o, d, tmin, tmax)
    hit = h["prim"] >= 0
    assert np.array_equal(hit, ref["hit"] != 0)
    assert np.array_equal(h["prim"], ref["prim"])
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(h[k]), bits(ref[k])), k
    assert np.array_equal(nv, ref["nodes"]) and np.array_equal(lv, ref["leaves"])
    # shadow queries (IS_SHADOW_RAY): the reference walks the same tree and records t alone; the
    # oracle's side of this comparison is its closest-hit trace (module docstring)
    assert np.array_equal(hit, ref["shadow_hit"] != 0)
    assert np.array_equal(bits(h["t"]), bits(ref["shadow_t"]))


@live
@pytest.mark.parametrize("model", RC.TRACE_MODELS)
def test_traversal_matches_the_reference(model):
    Os, Rs = RC.trace_scene(model, True)
    o, d, tmin, tmax, cls = RC.oracle_ray_set(model, Os)
    assert len(o) >= 10000 and set(cls) == set(RC.RAY_CLASSES)
    nodes, leaves = Rs.bvh_counts()
    info = Os.qbvh_info()
    assert (nodes, leaves) == (info["nodes"], info["leaves"])
    rec, sh = Rs.trace(o, d, tmin, tmax), Rs.trace(o, d, tmin, tmax, shadow=True)
    assert 0.2 < (rec["hit"] != 0).mean() < 0.98
    check_trace(Os, o, d, tmin, tmax, dict(hit=rec["hit"], t=rec["t"], a=rec["a"], b=rec["b"], prim=Rs.hit_ids(rec),
                                           nodes=rec["nodes"], leaves=rec["leaves"], shadow_hit=sh["hit"], shadow_t=sh["t"]))


@pytest.mark.parametrize("model", RC.TRACE_MODELS)
def test_traversal_matches_the_recorded_reference(model):
    fx = RC.fixture("trace_%s.npz" % model)
    Os, _ = RC.trace_scene(model, False)
    assert set(fx["cls"]) == set(range(len(RC.RAY_CLASSES)))
    info, rec = Os.qbvh_info(), RC.fixture_json()["bvh"][model]
    assert (info["nodes"], info["leaves"]) == (rec["nodes"], rec["leaves"])
    check_trace(Os, fx["o"], fx["d"], fx["tmin"], fx["tmax"], fx)
    # the recorded rays are rays of the set the live test traces
    o, d, tmin, tmax, cls = RC.oracle_ray_set(model, Os)
    keep = RC.fixture_subset(cls)
    assert same_bits(o[keep], fx["o"]) and same_bits(d[keep], fx["d"]) and same_bits(tmax[keep], fx["tmax"])


def test_ray_sets_hold_the_edge_cases():
    Os, _ = RC.trace_scene("cornell_box", False)
    o, d, tmin, tmax, cls = RC.oracle_ray_set("cornell_box", Os)
    z = d[cls == "zero_component"]
    nz = (z == 0).sum(1)
    assert set(nz) == {1, 2} and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    for k in ("tmax_at_t", "tmax_below_t", "tmax_above_t"):
        assert (cls == k).sum() >= 300


# ------------------------------------------------------------------ shading, exact
def oracle_frame(case, size=None):
    Os, _ = RC.build_scenes(case, False)
    w, h = size or RC.case_size(case)
    return Os.render(RC.case_camera(case), w, h, threads=4)["rgb"]


@live
@pytest.mark.parametrize("name", sorted(DET))
def test_deterministic_shading_matches_the_reference(name):
    case = DET[name]
    Os, Rs = RC.build_scenes(case, True)
    w, h = RC.case_size(case)
    assert same_bits(Os.render(RC.case_camera(case), w, h)["rgb"], Rs.render(RC.case_camera(case), w, h))


@live
@pytest.mark.parametrize("name", sorted(REPLAY))
def test_replayed_shading_matches_the_reference(name):
    case = REPLAY[name]
    Os, Rs = RC.build_scenes(case, True)
    w, h = RC.case_size(case)
    assert same_bits(Os.render(RC.case_camera(case), w, h)["rgb"], Rs.replay(RC.case_camera(case), w, h))


@pytest.mark.parametrize("name", ["deterministic." + n for n in sorted(DET)] + ["replay." + n for n in sorted(REPLAY)])
def test_shading_matches_the_recorded_reference(name):
    tier, key = name.split(".", 1)
    case = (DET if tier == "deterministic" else REPLAY)[key]
    ref = RC.fixture("frames.npz")[name]
    w, h = RC.case_size(case)
    assert ref.shape == (h, w, 3) and w <= 64 and h <= 64
    assert np.isfinite(ref).all() and np.unique(bits(ref)).size > 20      # a frame, not a constant
    assert same_bits(oracle_frame(case), ref)


def test_recorded_frames_are_the_cases_of_the_table():
    want = {"deterministic." + n for n in DET} | {"replay." + n for n in REPLAY}
    assert set(RC.fixture("frames.npz")) == want == set(RC.fixture_json()["frames"])


def test_replay_cases_do_what_their_names_say():
    """The noise threshold of the 8- and 16-sample rectangle lights stops some pixels early and
    lets others run: the frames differ from the 1-sample frame and from each other."""
    fr = RC.fixture("frames.npz")
    a, b, c = (fr["replay.rect_%d_fast" % n] for n in (1, 8, 16))
    assert not same_bits(a, b) and not same_bits(b, c)
    assert not same_bits(fr["replay.rect_8_fast"], fr["replay.rect_8_transparent"])
    for n in (8, 16):      # one shadow ray per light sample taken: fewer than n a pixel, more than n / 2's frame
        case = REPLAY["rect_%d_fast" % n]
        Os, _ = RC.build_scenes(case, False)
        r = Os.render(RC.case_camera(case), *RC.case_size(case))
        lit = int((r["hits"]["prim"] >= 0).sum())
        assert lit < r["shadow_rays"] < n * lit, (n, lit, r["shadow_rays"])


def test_depth_of_field_case_draws_a_varying_number_of_lens_samples():
    """Camera::eyeRayAdaptive rejects lens points outside the unit disc (src/Camera.cpp:164-168): on
    the replayed draws (dims 3, 4, then 5, 6, ... of each pixel) some pixels take the first pair and
    others need more (a pair lands in the disc with probability pi / 4), and the frame differs from the same camera with the aperture closed."""
    case = REPLAY["depth_of_field"]
    w, h = RC.case_size(case)
    L = O.lib()
    pairs = np.zeros(w * h, int)
    for p in range(w * h):
        k = 0
        while True:
            u, v = (np.float32(1.0 - np.float64(np.float32(2.0) * np.float32(L.oro_rand(p, 0, 3 + 2 * k + j, 0x5EED)))) for j in (0, 1))
            k += 1
            if not u * u + v * v > np.float32(1.0):
                break
        pairs[p] = k
    assert (pairs == 1).sum() > w * h // 2 and (pairs > 1).sum() > w * h // 10 and pairs.max() >= 3
    pinhole = dict(case, camera=dict(RC.case_camera(case), aperture=0.0))
    assert not same_bits(oracle_frame(pinhole), RC.fixture("frames.npz")["replay.depth_of_field"])


# ------------------------------------------------------------------ statistical tier
@live
@pytest.mark.parametrize("name", sorted(STAT))
def test_distribution_matches_the_reference(name):
    case = STAT[name]
    Os, Rs = RC.build_scenes(case, True)
    w, h = RC.STAT_SIZE
    K = RC.STAT_K
    reps = Rs.repeat(RC.case_camera(case), w, h, K + 1).astype(np.float64)
    m, s = reps[:K].mean(0), reps[:K].std(0, ddof=1)
    held = RC.statistics(reps[K], m, s, K)
    ours = RC.statistics(Os.render(RC.case_camera(case), w, h, threads=4)["rgb"], m, s, K)
    print(name, "held-out", held, "oracle", ours)
    RC.assert_statistics(held, "the reference's held-out replica")     # a condition of the test
    RC.assert_statistics(ours, "the oracle")


@pytest.mark.parametrize("name", sorted(STAT))
def test_distribution_matches_the_recorded_reference(name):
    fx, meta = RC.fixture("statistical.npz"), RC.fixture_json()["statistical"][name]
    m, s, K = fx[name + ".m"], fx[name + ".s"], meta["K"]
    assert K == RC.STAT_K and m.shape == RC.STAT_SIZE[::-1] + (3,)
    held = RC.statistics(fx[name + ".held_out"], m, s, K)
    ours = RC.statistics(oracle_frame(STAT[name], RC.STAT_SIZE), m, s, K)
    print(name, "held-out", held, "oracle", ours)
    RC.assert_statistics(held, "the reference's held-out replica")
    assert abs(held["bias"] - meta["held_out_bias"]) < 1e-5 and abs(held["max_z"] - meta["held_out_max_z"]) < 1e-5
    RC.assert_statistics(ours, "the oracle")


def test_z_bound_is_the_t_distribution_tail():
    # P(|t_63| > 2) = 0.04981 (tables); the bound at N = 3072 is "about 6"
    assert abs(RC.t_two_sided_tail(2.0, 63) - 0.0498) < 2e-4
    b = RC.z_bound(3072, 63)
    assert 5.5 < b < 6.0 and abs(3072 * RC.t_two_sided_tail(b, 63) - 1e-3) < 1e-6


# ------------------------------------------------------------------ deep tier: every chain level, replayed
_logged = {}


def deep_log(name):
    """The oracle's frame of a deep case with its draw log, rendered once and left unchanged."""
    if name not in _logged:
        case = DEEP[name]
        Os, _ = RC.build_scenes(case, False)
        _logged[name] = Os.render(RC.case_camera(case), *RC.case_size(case), threads=4, draw_log=True)
        for a in _logged[name].values():
            a.setflags(write=False)
    return _logged[name]


def pixel_of_draws(log):
    return np.repeat(np.arange(len(log["draw_offsets"]) - 1), np.diff(log["draw_offsets"]))


def explain(name, log, rgb, rgb8, draws):
    """None if the oracle's logged frame has these float bits, bytes and per-pixel draw counts; else
    the first differing pixel and its log decoded as (sample, path, level, branch, k)."""
    h, w = log["rgb"].shape[:2]
    n = np.diff(log["draw_offsets"]).reshape(h, w)
    bad = (bits(log["rgb"]) != bits(rgb)).any(2) | (log["rgb8"] != rgb8).any(2) | (n != draws)
    if not bad.any():
        return None
    y, x = (int(v) for v in np.argwhere(bad)[0])
    p = y * w + x
    keys = log["draw_keys"][log["draw_offsets"][p]:log["draw_offsets"][p + 1]]
    return "%s: %d pixels differ; first (x %d, y %d): oracle %r %r draws %d, reference %r %r draws %d; " \
           "log (sample, path, level, branch, k): %r" % (
               name, int(bad.sum()), x, y, log["rgb"][y, x].tolist(), log["rgb8"][y, x].tolist(), int(n[y, x]),
               np.asarray(rgb)[y, x].tolist(), np.asarray(rgb8)[y, x].tolist(), int(draws[y, x]), RC.decode_key(keys).tolist())


@live
@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_replay_matches_the_reference(name):
    """Float bits of the frame, the bytes Image::setPixel stored, and consumed == logged on every pixel."""
    case, log = DEEP[name], deep_log(name)
    _, Rs = RC.build_scenes(case, True)
    w, h = RC.case_size(case)
    ref = Rs.replay_log(RC.case_camera(case), w, h, log)
    Rs.close()
    why = explain(name, log, ref["rgb"], ref["rgb8"], ref["consumed"])
    assert why is None, why


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_replay_matches_the_recorded_reference(name):
    """Without the driver: the recorded frame, bytes and draw counts.  The oracle's log length of each
    pixel equals the number of draws the reference consumed there."""
    fx, log = RC.fixture("deep.npz"), deep_log(name)
    w, h = RC.case_size(DEEP[name])
    ref = fx[name + ".rgb"]
    assert ref.shape == (h, w, 3) and w <= 40 and h <= 36
    assert np.isfinite(ref).all() and np.unique(bits(ref)).size > 20
    meta = RC.fixture_json()["deep"]["frames"][name]
    assert RC.sha(ref) == meta["sha256"] and int(fx[name + ".draws"].max()) == meta["max_draws"]
    why = explain(name, log, ref, fx[name + ".rgb8"], fx[name + ".draws"].astype(np.int64))
    assert why is None, why


def test_recorded_deep_frames_are_the_cases_of_the_table():
    fx = RC.fixture("deep.npz")
    want = {n + s for n in DEEP for s in (".rgb", ".rgb8", ".draws")} | {"gamma.u8", "gamma.f32", "map.in", "map.out"}
    assert set(fx) == want and set(RC.fixture_json()["deep"]["frames"]) == set(DEEP)
    assert set(RC.fixture_json()["deep"]["decode"]) == set(RC.decode_images())


@pytest.mark.parametrize("name", sorted(DEEP))
def test_draw_log_leaves_the_frame_alone(name):
    """The log records; it takes no part in the arithmetic.  With any thread count (each pixel logs
    into storage of its own) the frame has the bits of the frame rendered without it."""
    case, log = DEEP[name], deep_log(name)
    Os, _ = RC.build_scenes(case, False)
    w, h = RC.case_size(case)
    plain = Os.render(RC.case_camera(case), w, h, threads=1)
    assert same_bits(plain["rgb"], log["rgb"]) and np.array_equal(plain["rgb8"], log["rgb8"])
    one = Os.render(RC.case_camera(case), w, h, threads=1, draw_log=True)
    assert np.array_equal(one["draw_keys"], log["draw_keys"]) and np.array_equal(one["draw_offsets"], log["draw_offsets"])
    assert len(log["draw_keys"]) == log["draw_offsets"][-1]


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_cases_reach_past_level_one(name):
    """From the oracle's log alone: level = (dim >> 24) - 1.  At least a tenth of the pixels draw at
    level >= 2, and no pixel comes near the 65536 draws at which the reference's pool wraps."""
    log = deep_log(name)
    d, pix = RC.decode_key(log["draw_keys"]), pixel_of_draws(log)
    n_pix = len(log["draw_offsets"]) - 1
    assert np.unique(pix[d[:, 2] >= 2]).size >= 0.10 * n_pix
    assert np.diff(log["draw_offsets"]).max() < 65536


def test_deep_cases_do_what_their_names_say():
    def parts(name):
        log = deep_log(name)
        return log, RC.decode_key(log["draw_keys"]), pixel_of_draws(log), len(log["draw_offsets"]) - 1
    for name in ("mirror_box", "glass_sphere"):      # the bounces < 5 cap is reached
        _, d, _, _ = parts(name)
        assert d[:, 2].max() == 5, name
    assert deep_log("glass_in_glass")["max_ior"].max() >= 3       # 1, 1.001, outer glass, inner glass
    log, d, pix, n_pix = parts("dispersion_sphere")
    per_branch = [np.unique(pix[d[:, 3] == b]) for b in (1, 2, 3)]
    assert np.intersect1d(np.intersect1d(per_branch[0], per_branch[1]), per_branch[2]).size >= 0.05 * n_pix
    log, d, pix, n_pix = parts("glossy_rect")
    assert np.unique(np.diff(log["draw_offsets"])).size >= 10
    # path tracing: a level's light draws come after its child's draws
    log, d, pix, n_pix = parts("path_trace_3")
    back = (pix[1:] == pix[:-1]) & (d[1:, 2] >= 0) & (d[1:, 2] + 1 == d[:-1, 2])
    assert np.unique(pix[1:][back]).size >= 0.10 * n_pix
    log, d, pix, n_pix = parts("num_paths_4")
    assert set(d[:, 1]) == {0, 1, 2, 3}
    assert not same_bits(log["rgb"], oracle_frame(dict(DEEP["num_paths_4"], num_paths=1)))
    # supersampling: 1 + 4 eye rays where the first level settles the pixel, 1 + 4 + 9 elsewhere; the lens
    # rejection loop (two draws a try after the three of jitter and time) takes a varying number of tries
    log, d, pix, n_pix = parts("supersampled_dof")
    eyes = np.array([np.unique(d[a:b, 0]).size for a, b in zip(log["draw_offsets"][:-1], log["draw_offsets"][1:])])
    assert set(eyes) == {5, 14} and (eyes == 5).sum() >= 10 and (eyes == 14).sum() >= 10
    cam = d[d[:, 2] == -1]
    per_ray = np.unique(np.stack([pix[d[:, 2] == -1], cam[:, 0]], 1), axis=0, return_counts=True)[1]
    assert ((per_ray - 3) % 2 == 0).all() and ((per_ray - 3) // 2).min() == 1 and ((per_ray - 3) // 2).max() >= 3


# ------------------------------------------------------------------ gamma tables, Map(), decoders
def check_gamma_and_map(u8, f32, x, mapped):
    assert u8.shape == (32769,) and f32.shape == (32769,)
    assert np.array_equal(O.gamma_table(), u8) and same_bits(O.gamma_table_f(), f32)
    assert np.array_equal(O.map_channel(x), mapped)


def test_map_inputs_are_the_listed_values():
    x = RC.map_inputs()
    assert len(x) == 2 + 3 * 512 + 4 and x[0] == 0 and x[1] == np.finfo(np.float32).tiny
    assert list(x[-4:]) == [1.0, np.nextafter(np.float32(1), np.float32(2)), 4.0, np.float32(1e30)]
    assert (x >= 0).all() and not np.isnan(x).any()
    k = x[2 + 512:2 + 1024] * 32768
    assert (k == np.round(k)).all() and np.unique(k).size == 512
    assert np.array_equal(bits(x[2:514]) + 1, bits(x[514:1026])) and np.array_equal(bits(x[514:1026]) + 1, bits(x[1026:1538]))


@live
def test_gamma_tables_and_map_match_the_reference():
    u8, f32 = refdriver.gamma_tables()
    x = RC.map_inputs()
    check_gamma_and_map(u8, f32, x, refdriver.map_values(x))


def test_gamma_tables_and_map_match_the_recorded_reference():
    fx = RC.fixture("deep.npz")
    assert same_bits(fx["map.in"], RC.map_inputs())
    check_gamma_and_map(fx["gamma.u8"], fx["gamma.f32"], fx["map.in"], fx["map.out"])


@live
@pytest.mark.parametrize("name", sorted(RC.decode_images()))
def test_decoder_matches_the_reference(name):
    path = RC.decode_images()[name]
    ours, theirs = RC.oracle_decode(path), refdriver.decode(path)
    assert ours.shape == theirs.shape and same_bits(ours, theirs)


@pytest.mark.parametrize("name", sorted(RC.decode_images()))
def test_decoder_matches_the_recorded_reference(name):
    ours, rec = RC.oracle_decode(RC.decode_images()[name]), RC.fixture_json()["deep"]["decode"][name]
    assert list(ours.shape) == rec["shape"] and RC.sha(ours) == rec["sha256"]
