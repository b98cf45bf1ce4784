"""Rebuild on the device against the host route, and what each tree costs a frame: what does
mrt_scene_rebuild_bvh cost next to mrt_scene_build_bvh + mrt_scene_upload, and how do a fresh
host build, a refitted tree and a rebuilt tree render the same geometry?  (One process, one
device; needs the GPU.)

    python tools/rebuild_bench.py [C3L C5 ...] [--rounds R] [--frame-rounds Q] [--out FILE]

Scenes: C3L (the 262 k-triangle Sponza stand-in as one world mesh) and C5 (64 instances of the
dragon / buddha stand-ins).  Per scene, after a clock-settle period of untimed frames, medians of
  build_upload_ms   wall time of mrt_scene_build_bvh + mrt_scene_upload (the host build is the
                    parent commit's: this change does not touch it)
  rebuild_ms        device events around the launches of the synchronous mrt_scene_rebuild_bvh
  rebuild_wall_ms   its wall time (wait, launches, wait, the topology read back)
  rebuild_async_ms  device events around mrt_scene_rebuild_bvh_async on the current stream
each rebuild after a refit to one of two small deformations, alternating (the first rebuild of
the replica, which allocates, is not timed); then for two deformations -- `small`: refit_bench's
1% of the extent (C3L) / instance_refit_bench's 2% shifts (C5); `large`: the mesh twisted by 90
degrees over its height (C3L) / the instances' positions permuted (C5) -- on three trees over
the same geometry
  frame_<tree>_ms   device time of a 1920x1080 frame (mrt_render_frame_async, K back to back),
                    the trees alternating
  cost_<tree>       mrt_scene_bvh_cost
with <tree> = fresh (a host build at the deformed geometry), refit (the built topology
refitted) and rebuilt (that tree after mrt_scene_rebuild_bvh), and the share of pixels whose hit
(prim, t) agrees between the rebuilt and the fresh tree.  Writes a JSON list (default
profiles/rebuild_bench.json) and prints one line per scene."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rendering-algorithms-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import miro  # noqa: E402
from miro import _lib, scenes  # noqa: E402
import refit_bench  # noqa: E402
import instance_refit_bench  # noqa: E402

SETTLE_S = 0.5


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def note(msg):
    print("[rebuild_bench] " + msg, file=sys.stderr, flush=True)


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def twisted(V):
    """V turned about the vertical axis through its box centre by 90 degrees times the height fraction."""
    lo, hi = V.min(0), V.max(0)
    c = 0.5 * (lo + hi)
    a = 0.5 * np.pi * (V[:, 1] - lo[1]) / max(float(hi[1] - lo[1]), 1e-12)
    x, z = V[:, 0] - c[0], V[:, 2] - c[2]
    out = V.astype(np.float64).copy()
    out[:, 0] = c[0] + np.cos(a) * x - np.sin(a) * z
    out[:, 2] = c[2] + np.sin(a) * x + np.cos(a) * z
    return np.ascontiguousarray(out, np.float32)


def permuted(mats, seed):
    """Each instance at another instance's position: its matrix translated there."""
    rng = np.random.default_rng(seed)
    p = np.array([np.asarray(M, np.float64)[:3, 3] / np.asarray(M, np.float64)[3, 3] for M in mats])
    order = rng.permutation(len(mats))
    out = np.empty((len(mats), 4, 4), np.float32)
    for i, M in enumerate(mats):
        T = np.eye(4)
        T[:3, 3] = p[order[i]] - p[i]
        out[i] = (T @ np.asarray(M, np.float64)).astype(np.float32)
    return out


class MeshCase:
    """C3L: the deformations are vertex sets of mesh 0."""
    key = "C3L"

    def __init__(self):
        self.scene, self.cam, self.W, self.H = refit_bench.build(self.key)
        self.refit, _, _, _ = refit_bench.build(self.key)
        V0 = self.scene.mesh_arrays(0)[0]
        amp = 0.01 * float((V0.max(0) - V0.min(0)).max())
        self.small = [refit_bench.displaced(V0, 1, amp), refit_bench.displaced(V0, 2, amp)]
        self.large = twisted(V0)

    def apply(self, scene, x):
        return scene.updateMesh(0, x)

    def fresh(self, x):
        return refit_bench.build(self.key, x)[0]


class InstanceCase:
    """C5: the deformations are the 64 instance matrices."""
    key = "C5"

    def __init__(self):
        self.scene, self.cam, cfg = scenes.build_config(self.key)
        self.refit, _, _ = scenes.build_config(self.key)
        self._fresh, _, _ = scenes.build_config(self.key)
        self.W, self.H = cfg["W"], cfg["H"]
        n = self.scene.instance_count()
        M0 = [self.scene.instance_info(i)["m"] for i in range(n)]
        ex = self.scene.bvh_export()[0][0].reshape(6, 4)
        shift = 0.02 * float((ex[3:].max(1) - ex[:3].min(1)).min())
        self.small = [instance_refit_bench.moved(M0, 1, shift), instance_refit_bench.moved(M0, 2, shift)]
        self.large = permuted(M0, 3)

    def apply(self, scene, x):
        return scene.updateInstances(x)

    def fresh(self, x):   # one scene object, built again at the new matrices
        for p, Mi in zip(instance_refit_bench.proxies(self._fresh), x):
            p.matrix = Mi.copy()
        self._fresh.preCalc()
        return self._fresh


def measure(case, rounds, frame_rounds, frame_reps):
    L = miro.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene, cam, W, H = case.scene, case.cam, case.W, case.H
    h = scene.handle
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

    built = dict(scene.bvh_info)
    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    render(scene)
    torch.cuda.synchronize()
    settle([scene])
    route, build_ms = [], []
    for _ in range(max(3, rounds // 3)):   # the host route (the frame after it is not timed)
        t0 = time.perf_counter()
        _lib.check(L.mrt_scene_build_bvh(h), "build")
        t1 = time.perf_counter()
        _lib.check(L.mrt_scene_upload(h, 0), "upload")
        torch.cuda.synchronize()
        route.append((time.perf_counter() - t0) * 1e3)
        build_ms.append((t1 - t0) * 1e3)
        render(scene)
        torch.cuda.synchronize()
    note("%s: host route timed" % case.key)
    case.apply(scene, case.small[0])
    scene.rebuildBVH()   # the first rebuild of a replica allocates: not timed
    settle([scene])
    dev_ms, wall = [], []
    for r in range(rounds):
        case.apply(scene, case.small[(r + 1) % 2])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = scene.rebuildBVH()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(ms)
        render(scene)
        torch.cuda.synchronize()
    asyn = []
    st = torch.cuda.current_stream(dev)
    for r in range(rounds):
        case.apply(scene, case.small[(r + 1) % 2])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scene.rebuildBVH(stream=st)
        e1.record()
        e1.synchronize()
        asyn.append(e0.elapsed_time(e1))
        render(scene)
        torch.cuda.synchronize()
    note("%s: rebuild timed" % case.key)
    out = {"scene": case.key, "world_prims": built["prims"], "built_nodes": built["nodes"], "built_leaves": built["leaves"],
           "W": W, "H": H, "rounds": rounds, "frame_rounds": frame_rounds, "frame_reps": frame_reps,
           "library": _lib.build_info(L)["library"],
           "build_upload_ms": med(route), "build_ms": med(build_ms), "rebuild_ms": med(dev_ms), "rebuild_wall_ms": med(wall),
           "rebuild_async_ms": med(asyn)}
    out["route_over_rebuild_wall"] = round(out["build_upload_ms"]["median"] / out["rebuild_wall_ms"]["median"], 1)
    _lib.check(L.mrt_scene_upload(case.refit.handle, 0), "upload")
    for name, x in (("small", case.small[0]), ("large", case.large)):
        case.apply(case.refit, x)          # the built topology, refitted
        case.apply(scene, x)               # the same, then rebuilt
        scene.rebuildBVH()
        fresh = case.fresh(x)
        _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")
        trees = (("fresh", fresh), ("refit", case.refit), ("rebuilt", scene))
        d = {"cost_" + k: round(s.bvhCost(), 3) for k, s in trees}
        d["rebuilt_nodes"], d["rebuilt_leaves"] = scene.bvh_info["nodes"], scene.bvh_info["leaves"]
        img_r, img_f = miro.Image(), miro.Image()
        img_r.resize(W, H); img_f.resize(W, H)
        hr = scene.raytraceImage(cam, img_r, want_hits=True)
        hf = fresh.raytraceImage(cam, img_f, want_hits=True)
        agree = (hr["prim"] == hf["prim"]) & (hr["t"].view(np.uint32) == hf["t"].view(np.uint32))
        d["hits_agree_rebuilt_fresh"] = round(float(agree.mean()), 6)
        settle([s for _, s in trees])
        frames = {k: [] for k, _ in trees}
        for q in range(frame_rounds):
            for k, s in trees:
                render(s)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(frame_reps):
                    render(s)
                e1.record()
                e1.synchronize()
                frames[k].append(e0.elapsed_time(e1) / frame_reps)
        for k, _ in trees:
            d["frame_%s_ms" % k] = med(frames[k])
        d["frame_refit_over_fresh"] = round(d["frame_refit_ms"]["median"] / d["frame_fresh_ms"]["median"], 4)
        d["frame_rebuilt_over_fresh"] = round(d["frame_rebuilt_ms"]["median"] / d["frame_fresh_ms"]["median"], 4)
        d["frame_rebuilt_over_refit"] = round(d["frame_rebuilt_ms"]["median"] / d["frame_refit_ms"]["median"], 4)
        out[name] = d
        note("%s: %s deformation measured" % (case.key, name))
    return out


def main():
    if miro.device_count() < 1:
        raise SystemExit("rebuild_bench.py: no HIP device visible (timings need the GPU)")
    cases = {"C3L": MeshCase, "C5": InstanceCase}
    keys = [a for a in sys.argv[1:] if a in cases] or list(cases)
    rounds, frame_rounds, frame_reps = opt("--rounds", 9), opt("--frame-rounds", 5), opt("--frame-reps", 5)
    path = opt("--out", os.path.join(ROOT, "profiles", "rebuild_bench.json"))
    results = []
    for key in keys:
        results.append(measure(cases[key](), rounds, frame_rounds, frame_reps))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
