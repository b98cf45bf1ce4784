"""The wavefront form of the light query against the fused one: what does mrt_light_samples_async
cost next to mrt_sample_lights_async and mrt_shade_hits_async?  (One process, one device; needs the GPU.)

    python tools/light_samples_ab.py [C3 C4 C5 ...] [--rounds R] [--reps K] [--out FILE] [--only e,fused]

Per config, at its own frame size, with device buffers throughout, on the config's white-Lambert
twin (tools/sample_lights_ab.py: the one scene on which mrt_shade_hits computes the same numbers),
at the points and normals mrt_hit_surfaces_async gives for the camera's own rays:
  shade     mrt_shade_hits_async on those rays and hits (conversion, gen, binned shadow rays, resolve)
  fused     mrt_sample_lights_async, e alone: one kernel, a lane per point, nothing binned
  e         mrt_light_samples_async, e alone: gen / bin / trace / resolve, records in scratch
  records   mrt_light_samples_async, samples + counts
  all       mrt_light_samples_async, samples + counts + e + per_light
Before timing, e of "fused", "e" and "all" is compared bit for bit (and with the shaded frame on
every hit row), per_light of "all" with mrt_sample_lights_async's, and the shadow-ray counts are
recorded.  The variants alternate within each round after a clock-settle period and a warm-up
of each; a sample is the HIP-event time of K back-to-back calls on one stream, divided by K.
Prints one JSON line per config; --out appends them to a file.  --only keeps the named variants
(a kernel trace of one dispatch: rocprofv3 --kernel-trace --stats -- python tools/light_samples_ab.py
C5 --only e --rounds 1); the comparisons then cover the variants that ran."""
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
from miro import _lib  # noqa: E402
from sample_lights_ab import SETTLE_S, opt, white_twin  # noqa: E402
from miro import scenes  # noqa: E402


def measure(key, rounds, reps, only=()):
    L = miro.lib()
    scene, cam, cfg = white_twin(key)
    W, H = cfg["W"], cfg["H"]
    n = W * H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    o, d, t = (torch.from_numpy(x).to(dev) for x in cam.rays(W, H))
    lo = torch.full((n,), 0.001, dtype=torch.float32, device=dev)
    hi = torch.full((n,), 1e12, dtype=torch.float32, device=dev)
    hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
    surf = torch.empty((n, 21), dtype=torch.int32, device=dev)
    h = scene.handle
    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    _lib.check(L.mrt_trace_rays_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, 0,
                                      hits.data_ptr(), stream), "trace_rays")
    _lib.check(L.mrt_hit_surfaces_async(h, o.data_ptr(), d.data_ptr(), hits.data_ptr(), n, surf.data_ptr(), stream),
               "hit_surfaces")
    words = surf.view(torch.float32)   # mrt_surface: p at words 0-2, n at 3-5
    p, nrm = words[:, 0:3].contiguous(), words[:, 3:6].contiguous()
    nl, m = len(scene._lights), scene.lightSampleCap()[1]
    f32 = dict(dtype=torch.float32, device=dev)
    rgb, e_fused, e_wave, e_all = (torch.empty((n, 3), **f32) for _ in range(4))
    per_fused, per_all = torch.empty((n, nl, 4), **f32), torch.empty((n, nl, 4), **f32)
    rec = torch.zeros((n, m, 8), **f32)
    counts = torch.zeros((n, nl), dtype=torch.int32, device=dev)

    def shade():
        _lib.check(L.mrt_shade_hits_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), hits.data_ptr(), n, W, 0, 0,
                                          rgb.data_ptr(), stream), "shade_hits")

    def fused(per=None):
        _lib.check(L.mrt_sample_lights_async(h, p.data_ptr(), nrm.data_ptr(), None, t.data_ptr(), n, 0, 0, 0, 0,
                                             e_fused.data_ptr(), per, stream), "sample_lights")

    def wave(samples, cnt, e, per):
        _lib.check(L.mrt_light_samples_async(h, p.data_ptr(), nrm.data_ptr(), None, t.data_ptr(), n, 0, 0, 0, 0,
                                             samples, cnt, e, per, stream), "light_samples")

    variants = {
        "shade": shade,
        "fused": fused,
        "e": lambda: wave(None, None, e_wave.data_ptr(), None),
        "records": lambda: wave(rec.data_ptr(), counts.data_ptr(), None, None),
        "all": lambda: wave(rec.data_ptr(), counts.data_ptr(), e_all.data_ptr(), per_all.data_ptr()),
    }
    variants = {k: f for k, f in variants.items() if not only or k in only}
    # same bits first (also the warm-up of every variant's kernels and scratch)
    rays = {}
    for name, f in variants.items():
        f()
        rays[name] = int(scene.stats()["shadow_rays"])
    fused(per_fused.data_ptr())
    torch.cuda.synchronize()
    hit = (hits[:, 3] >= 0).cpu().numpy()
    a = e_fused.cpu().numpy().view(np.uint32)
    if "shade" in variants:
        assert np.array_equal(a[hit], rgb.cpu().numpy().view(np.uint32)[hit]), "fused e differs from the shaded frame"
    for name, x in (("e", e_wave), ("all", e_all)):
        if name in variants:
            b = x.cpu().numpy().view(np.uint32)
            assert np.array_equal(a, b), "%s: e differs from mrt_sample_lights on %d of %d points" % (name, (a != b).any(1).sum(), n)
    if "all" in variants:
        assert torch.equal(per_fused.view(torch.int32), per_all.view(torch.int32)), "per_light differs from mrt_sample_lights"
    fused_rays = int(scene.stats()["shadow_rays"])
    assert all(v == fused_rays for k, v in rays.items() if k != "shade"), rays
    taken = int(counts.sum().item())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < SETTLE_S:   # clock settle: untimed work
        for f in variants.values():
            f()
        torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            f()   # this variant's warm-up after the previous one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) / reps)
    ms = {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
          for k, v in samples.items()}
    med = {k: v["median"] for k, v in ms.items()}
    ratio = lambda a, b: round(med[a] / med[b], 4) if a in med and b in med else None
    return {"config": key, "twin": "white Lambert, 1 path", "W": W, "H": H, "points": n, "hit_rows": int(hit.sum()),
            "lights": nl, "rows_per_point": m, "samples_taken": taken, "rounds": rounds, "reps": reps,
            "library": _lib.build_info(L)["library"], "ms": ms, "shadow_rays": rays,
            "e_over_fused": ratio("e", "fused"), "e_over_shade": ratio("e", "shade"), "all_over_e": ratio("all", "e")}


def main():
    if miro.device_count() < 1:
        raise SystemExit("light_samples_ab.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in scenes.CONFIGS] or ["C3", "C4", "C5"]
    rounds, reps, path = opt("--rounds", 9), opt("--reps", 10), opt("--out", "")
    only = tuple(x for x in opt("--only", "").split(",") if x)
    for key in keys:
        line = json.dumps(measure(key, rounds, reps, only))
        print(line, flush=True)
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
