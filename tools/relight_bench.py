"""Relighting in place against the route it replaces: what do mrt_scene_update_lights /
_material / _texture cost next to a re-upload (an old setter marks the scene dirty, then
mrt_scene_upload) or, for a new sky, a new scene?  (One process, one device; needs the GPU.)

    python tools/relight_bench.py [D1 C5 ...] [--rounds R] [--out FILE]
    python tools/relight_bench.py D1 --updates N     # N async texture updates only, for a kernel trace

Scenes: D1 and C5 at their own sky (a dome light and the environment map on one texture).
Per scene, first the check: one frame after updateTexture / updateLights / updateMaterial
against one frame of a scene built fresh with the same values must be equal bits.  Then, after
a clock-settle period of untimed frames, medians over R rounds of
  reupload_ms         wall time of an old setter (mrt_scene_set_material_sample_env: the scene
                      goes dirty) + mrt_scene_upload: every replica freed, the host image rebuilt,
                      every array copied again
  new_scene_ms        wall time of preCalc() with the new sky + mrt_scene_upload: the only route
                      to new texels there was
  lights_wall_ms / lights_dev_ms        updateLights: synchronous wall time; device events
                      around the async form
  material_wall_ms / material_dev_ms    updateMaterial, the same
  texture_wall_ms / texture_update_ms   updateTexture of a numpy array: wall time; the device
                      time it returns (copy in excluded: events around the kernels)
  texture_async_ms    device events around updateTexture of a device tensor
  frame_updated_ms / frame_fresh_ms     device time of a frame on the updated scene and on the
                      fresh one, alternating
Writes a JSON list (default profiles/relight_bench.json) and prints one line per scene."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rendering-algorithms-raytracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import miro  # noqa: E402
from miro import _lib, scenes  # noqa: E402

SETTLE_S = 0.5
FRAME_REPS = 5


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def skies(rgb):
    """Two other skies of the same size: the sky turned by a seventh of a turn and dimmed, and
    turned the other way and brightened."""
    w = rgb.shape[1]
    return (np.ascontiguousarray(np.roll(rgb, w // 7, axis=1) * np.float32(0.6)),
            np.ascontiguousarray(np.roll(rgb, -(w // 5), axis=1) * np.float32(1.3)))


def relit(scene, k):
    """The light and material values of variant k on the scene's objects."""
    dome = scene._lights[0]
    dome.setPower(0.15 if k == 0 else 0.22)
    dome.setSamples(6 if k == 0 else 4)
    mat = list(scene._mat_objs.values())[0]
    mat.setKd((1, 1, 1) if k == 0 else (0.8, 0.7, 0.5))
    return mat


def measure(key, rounds):
    L = miro.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene, cam, cfg = scenes.build_config(key)
    W, H = cfg["W"], cfg["H"]
    h = scene.handle
    tex = scene._lights[0].texture
    sky0 = tex.m_image.m_rawData
    sky_a, sky_b = skies(sky0)
    rgb = torch.empty(H * W * 3, dtype=torch.float32, device=dev)
    cc = cam._c()
    opts = _lib.mrt_render_opts(W, H, 0, 0, 0, 0, 0)

    def render(s):
        _lib.check(L.mrt_render_frame_async(s.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), None, stream), "frame")

    def frame_bits(s):
        render(s)
        torch.cuda.synchronize()
        return rgb.cpu().numpy().view(np.uint32).copy()

    def settle(ss):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < SETTLE_S:
            for s in ss:
                render(s)
            torch.cuda.synchronize()

    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    frame_bits(scene)
    # the check, before anything is timed: the updated scene against a scene built with the same values
    scene.updateTexture(tex, sky_a)
    mat = relit(scene, 1)
    scene.updateLights()
    scene.updateMaterial(mat)
    updated = frame_bits(scene)
    fresh, _, _ = scenes.build_config(key)
    fresh._lights[0].texture.m_image.m_rawData = sky_a
    relit(fresh, 1)
    t0 = time.perf_counter()
    fresh.preCalc()
    _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")
    torch.cuda.synchronize()
    new_scene = [(time.perf_counter() - t0) * 1e3]
    equal = bool(np.array_equal(updated, frame_bits(fresh)))
    if not equal:
        raise SystemExit(f"relight_bench.py: {key}: the frame after the updates differs from the fresh scene's")
    uploads0 = scene.uploadCount()
    settle([scene])
    reupload = []
    for _ in range(rounds):   # the route before these entries
        t0 = time.perf_counter()
        _lib.check(L.mrt_scene_set_material_sample_env(h, 0, 1), "old setter")
        _lib.check(L.mrt_scene_upload(h, 0), "upload")
        torch.cuda.synchronize()
        reupload.append((time.perf_counter() - t0) * 1e3)
        render(scene)
        torch.cuda.synchronize()
    assert scene.uploadCount() == uploads0 + rounds
    scene.updateTexture(tex, sky_b)   # the first texture update of the new replica allocates: not timed
    settle([scene])
    out = {}

    def timed(name, sync, asyn):
        wall, devms = [], []
        for r in range(rounds):
            t0 = time.perf_counter()
            sync(r)
            wall.append((time.perf_counter() - t0) * 1e3)
            render(scene)
            torch.cuda.synchronize()
        for r in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            asyn(r)
            e1.record()
            e1.synchronize()
            devms.append(e0.elapsed_time(e1))
            render(scene)
            torch.cuda.synchronize()
        out[name + "_wall_ms"], out[name + "_dev_ms"] = med(wall), med(devms)

    def lights(r, **kw):
        relit(scene, r % 2)
        scene.updateLights(**kw)

    def material(r, **kw):
        scene.updateMaterial(relit(scene, r % 2), **kw)

    timed("lights", lights, lambda r: lights(r, asynchronous=True))
    timed("material", material, lambda r: material(r, asynchronous=True))
    wall, upd = [], []
    for r in range(rounds):
        t0 = time.perf_counter()
        ms = scene.updateTexture(tex, sky_a if r % 2 == 0 else sky_b)
        wall.append((time.perf_counter() - t0) * 1e3)
        upd.append(ms)
        render(scene)
        torch.cuda.synchronize()
    ta, tb = torch.from_numpy(sky_a).to(dev), torch.from_numpy(sky_b).to(dev)
    torch.cuda.synchronize()
    asyn = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scene.updateTexture(tex, ta if r % 2 == 0 else tb)
        e1.record()
        e1.synchronize()
        asyn.append(e0.elapsed_time(e1))
        render(scene)
        torch.cuda.synchronize()
    assert scene.textureUpdateStatus() == 0 and scene.uploadCount() == uploads0 + rounds
    # frames: the updated scene against the fresh one, at the same values again
    scene.updateTexture(tex, sky_a)
    mat = relit(scene, 1)
    scene.updateLights()
    scene.updateMaterial(mat)
    equal_after = bool(np.array_equal(frame_bits(scene), frame_bits(fresh)))
    settle([scene, fresh])
    frames = {"updated": [], "fresh": []}
    for _ in range(rounds):
        for name, s in (("updated", scene), ("fresh", fresh)):
            render(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(FRAME_REPS):
                render(s)
            e1.record()
            e1.synchronize()
            frames[name].append(e0.elapsed_time(e1) / FRAME_REPS)
    res = {"scene": key, "W": W, "H": H, "sky": [int(sky0.shape[1]), int(sky0.shape[0])], "rounds": rounds,
           "library": _lib.build_info(L)["library"], "frame_equals_fresh_scene": equal,
           "frame_equals_fresh_scene_after_timing": equal_after,
           "reupload_ms": med(reupload), "new_scene_ms": med(new_scene)}
    res.update(out)
    res.update({"texture_wall_ms": med(wall), "texture_update_ms": med(upd), "texture_async_ms": med(asyn),
                "frame_updated_ms": med(frames["updated"]), "frame_fresh_ms": med(frames["fresh"])})
    res["reupload_over_texture_wall"] = round(res["reupload_ms"]["median"] / res["texture_wall_ms"]["median"], 1)
    res["reupload_over_lights_wall"] = round(res["reupload_ms"]["median"] / res["lights_wall_ms"]["median"], 1)
    return res


def updates_only(key, n):
    """n async texture updates and nothing else timed: the run a kernel trace is taken of."""
    scene, cam, cfg = scenes.build_config(key)
    _lib.check(miro.lib().mrt_scene_upload(scene.handle, 0), "upload")
    tex = scene._lights[0].texture
    dev = torch.device("cuda", 0)
    ts = [torch.from_numpy(s).to(dev) for s in skies(tex.m_image.m_rawData)]
    for r in range(n + 1):
        scene.updateTexture(tex, ts[r % 2])
        torch.cuda.synchronize()
    print("relight_bench.py: %d texture updates on %s, %d refused" % (n + 1, key, scene.textureUpdateStatus()))


def main():
    if miro.device_count() < 1:
        raise SystemExit("relight_bench.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in ("D1", "C5")] or ["D1", "C5"]
    if "--updates" in sys.argv:
        return updates_only(keys[0], opt("--updates", 9))
    rounds = opt("--rounds", 9)
    path = opt("--out", os.path.join(ROOT, "profiles", "relight_bench.json"))
    results = []
    for key in keys:
        results.append(measure(key, rounds))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
