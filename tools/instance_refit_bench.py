"""Instance refit against rebuild: what does mrt_scene_update_instances cost next to the only
route there was before it, a new scene at the new matrices + mrt_scene_build_bvh +
mrt_scene_upload?  (One process, one device; needs the GPU.)

    python tools/instance_refit_bench.py [C5 FS ...] [--rounds R] [--frame-rounds Q] [--frame-reps K] [--out FILE]

Scenes: C5 (64 instances of the dragon / 1.09 M-triangle buddha stand-ins) and FS (the
reference's final scene, 42 k instances).  Every instance is moved by a seeded rigid transform
about its own position (a rotation of up to 20 degrees, a shift of up to 2% of the scene's
extent), the updates alternating between two such sets.  Per scene, after a clock-settle
period of untimed frames, medians over R rounds of
  refit_ms           device events around the kernels of the synchronous entry (the instance
                     kernel, the leaf kernel, one node kernel per height)
  refit_wall_ms      wall time of the synchronous mrt_scene_update_instances
  refit_async_ms     device events around mrt_scene_update_instances_async on a device tensor
  rebuild_upload_ms  the route it replaces, in the same run: a second scene object given the new
                     matrices, everything added again (the BLAS builds included), then
                     mrt_scene_build_bvh and mrt_scene_upload; world_build_ms / blas_build_ms
                     are the two builds inside it
  frame_refit_ms / frame_fresh_ms   device time of a frame (mrt_render_frame_async, K back to
                     back) on the refitted tree and on the fresh build at the same matrices,
                     alternating (Q rounds, default R: a frame of FS takes seconds)
the share of pixels whose hit (prim, t) agrees between the two trees, and whether the
instances the device holds after the refit equal the fresh scene's bit for bit.  Writes a JSON
list (default profiles/instance_refit_bench.json) and prints one line per scene."""
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
FRAME_REPS = 3


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def note(msg):
    print("[instance_refit_bench] " + msg, file=sys.stderr, flush=True)


def proxies(scene):
    return [e[0] for e in scene._meshes if isinstance(e[0], miro.ProxyObject)]


def moved(mats, seed, shift):
    """Each matrix under a seeded rigid transform about its own position: T(p + d) R T(-p) M."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(mats), 4, 4), np.float32)
    for i, M in enumerate(mats):
        M = np.asarray(M, np.float64)
        p = M[:3, 3] / M[3, 3]
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        th = rng.uniform(-1, 1) * np.radians(20.0)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(4)
        R[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        R[:3, 3] = p + rng.uniform(-shift, shift, 3) - R[:3, :3] @ p
        out[i] = (R @ M).astype(np.float32)
    return out


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def measure(key, rounds, frame_rounds, frame_reps):
    L = miro.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene, cam, cfg = scenes.build_config(key)
    fresh, _, _ = scenes.build_config(key)   # the second scene object: rebuilt at the new matrices
    W, H = cfg["W"], cfg["H"]
    n = scene.instance_count()
    note("%s: two scenes built, %d instances" % (key, n))
    M0 = [scene.instance_info(i)["m"] for i in range(n)]
    ex = scene.bvh_export()[0][0].reshape(6, 4)
    shift = 0.02 * float((ex[3:].max(1) - ex[:3].min(1)).min())
    Ma, Mb = moved(M0, 1, shift), moved(M0, 2, shift)
    rgb = torch.empty(H * W * 3, dtype=torch.float32, device=dev)
    cc = cam._c()
    opts = _lib.mrt_render_opts(W, H, 0, 0, 0, 0, 0)

    def render(s):
        _lib.check(L.mrt_render_frame_async(s.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), None, stream), "frame")

    def settle(ss):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < SETTLE_S:
            for s in ss:
                render(s)
            torch.cuda.synchronize()

    _lib.check(L.mrt_scene_upload(scene.handle, 0), "upload")
    render(scene)
    torch.cuda.synchronize()
    scene.updateInstances(Ma)   # the first refit of a replica makes its schedule: not timed
    settle([scene])
    refit, wall = [], []
    for r in range(rounds):
        m = Mb if r % 2 == 0 else Ma
        t0 = time.perf_counter()
        ms = scene.updateInstances(m)
        wall.append((time.perf_counter() - t0) * 1e3)
        refit.append(ms)
        render(scene)
        torch.cuda.synchronize()
    ta, tb = torch.from_numpy(Ma).to(dev), torch.from_numpy(Mb).to(dev)
    torch.cuda.synchronize()
    asyn = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scene.updateInstances(tb if r % 2 == 0 else ta)
        e1.record()
        e1.synchronize()
        asyn.append(e0.elapsed_time(e1))
        render(scene)
        torch.cuda.synchronize()
    note("%s: refit timed" % key)
    rebuild, world, blas = [], [], []
    for r in range(max(2, rounds // 3)):   # the route before this entry (the frame after it is not timed)
        m = Mb if r % 2 == 0 else Ma
        t0 = time.perf_counter()
        for p, Mi in zip(proxies(fresh), m):
            p.matrix = Mi.copy()
        fresh.preCalc()
        _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")
        torch.cuda.synchronize()
        rebuild.append((time.perf_counter() - t0) * 1e3)
        world.append(fresh.bvh_build_ms)
        blas.append(fresh.blas_build_ms)
        render(fresh)
        torch.cuda.synchronize()
    note("%s: rebuild route timed" % key)
    # frames: the refitted tree at Ma against the fresh build at Ma
    scene.updateInstances(ta)
    for p, Mi in zip(proxies(fresh), Ma):
        p.matrix = Mi.copy()
    fresh.preCalc()
    _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")
    same = all(np.array_equal(scene.instance_info(i)[k].view(np.uint32), fresh.instance_info(i)[k].view(np.uint32))
               for i in range(n) for k in ("m", "inv", "inv_t", "box"))
    img_r, img_f = miro.Image(), miro.Image()
    img_r.resize(W, H); img_f.resize(W, H)
    hr = scene.raytraceImage(cam, img_r, want_hits=True)
    hf = fresh.raytraceImage(cam, img_f, want_hits=True)
    agree = (hr["prim"] == hf["prim"]) & (hr["t"].view(np.uint32) == hf["t"].view(np.uint32))
    note("%s: hits compared" % key)
    settle([scene, fresh])
    frames = {"refit": [], "fresh": []}
    for q in range(frame_rounds):
        note("%s: frames, round %d of %d" % (key, q + 1, frame_rounds))
        for name, s in (("refit", scene), ("fresh", fresh)):
            render(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(frame_reps):
                render(s)
            e1.record()
            e1.synchronize()
            frames[name].append(e0.elapsed_time(e1) / frame_reps)
    info = scene.bvh_info
    out = {"scene": key, "instances": n, "world_prims": info["prims"], "nodes": info["nodes"], "leaves": info["leaves"],
           "node_launches": info["max_depth"], "blas_prims": scene.blas_prims, "W": W, "H": H, "rounds": rounds, "frame_rounds": frame_rounds, "frame_reps": frame_reps,
           "shift": round(shift, 5), "library": _lib.build_info(L)["library"],
           "refit_ms": med(refit), "refit_wall_ms": med(wall), "refit_async_ms": med(asyn),
           "rebuild_upload_ms": med(rebuild), "world_build_ms": med(world), "blas_build_ms": med(blas),
           "frame_refit_ms": med(frames["refit"]), "frame_fresh_ms": med(frames["fresh"]),
           "hits_agree": round(float(agree.mean()), 6), "device_instances_equal_fresh_scene": bool(same)}
    out["rebuild_over_refit_wall"] = round(out["rebuild_upload_ms"]["median"] / out["refit_wall_ms"]["median"], 1)
    out["frame_refit_over_fresh"] = round(out["frame_refit_ms"]["median"] / out["frame_fresh_ms"]["median"], 4)
    return out


def main():
    if miro.device_count() < 1:
        raise SystemExit("instance_refit_bench.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in ("C5", "FS")] or ["C5", "FS"]
    rounds = opt("--rounds", 9)
    frame_rounds, frame_reps = opt("--frame-rounds", rounds), opt("--frame-reps", FRAME_REPS)
    path = opt("--out", os.path.join(ROOT, "profiles", "instance_refit_bench.json"))
    results = []
    for key in keys:
        results.append(measure(key, rounds, frame_rounds, frame_reps))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
