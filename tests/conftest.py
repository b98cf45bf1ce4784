import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rendering-algorithms-raytracer_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def ref_model(rel):
    """Path of one of the reference's model files, from this repository's own copies: the
    small meshes under tests/golden/models, Final/<name> from assets/final (unpacked into
    the scene cache and checked against its manifest's sha256)."""
    if rel.startswith("Final/"):
        from miro import final_scene
        return final_scene.asset(rel[len("Final/"):])
    return os.path.join(GOLDEN, "models", rel)


TOPANGA_SHA256 = "b1bdb63224034b68290098de1e568a0aa5d499475460a97526c6ab50258256a3"


def _unpacked_golden(name, sha256):
    """tests/golden/<name>.xz unpacked into the scene cache (sha256 checked)."""
    import hashlib
    import lzma
    from miro import scenes
    out = os.path.join(scenes._cache_dir(), sha256[:12] + "_" + name)
    if not os.path.exists(out):
        data = lzma.decompress(open(os.path.join(GOLDEN, name + ".xz"), "rb").read())
        assert hashlib.sha256(data).hexdigest() == sha256, name
        tmp = out + ".tmp%d" % os.getpid()
        open(tmp, "wb").write(data)
        os.replace(tmp, out)
    return out


def ref_hdr_images():
    """The reference's .hdr files this repository holds: four of the six Images/*.hdr and the
    final scene's Textures/hdrvfx_*.hdr.  The other two, Mono_Lake.hdr (3.8 MB; 2.8 MB
    xz-packed) and rnl_probe.hdr (2.2 MB; 1.7 MB xz-packed), stay above the 1 MiB a
    committed file may have however they are packed.  {name: path}."""
    from miro import final_scene, scenes
    return {"Arches_E_PineTree.hdr": scenes.ARCHES_HDR,
            "Arches_E_PineTree_Env.hdr": os.path.join(GOLDEN, "Arches_E_PineTree_Env.hdr"),
            "Topanga_Forest_B_light.hdr": _unpacked_golden("Topanga_Forest_B_light.hdr", TOPANGA_SHA256),
            "sky.hdr": final_scene.asset("sky.hdr"),
            "hdrvfx_nyany_1_n2_v101_Ref.hdr": final_scene.asset("hdrvfx_nyany_1_n2_v101_Ref.hdr")}


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device)")
    config.addinivalue_line("markers", "slow: long-running CPU check")


@pytest.fixture(scope="session")
def golden():
    return GOLDEN


@pytest.fixture(scope="session", autouse=True)
def _oracle_reference_libm():
    """Every GPU-vs-oracle comparison uses the reference's libm convention (glibc's atan2f /
    acosf / sinf / cosf / powf, oracle.LIBM_FLOAT): the device restates those five functions
    bit for bit (csrc/mrt_libm.h, pinned by tests/test_libm.py)."""
    import oracle
    prev = oracle.set_default_libm(oracle.LIBM_FLOAT)
    yield
    oracle.set_default_libm(prev)
