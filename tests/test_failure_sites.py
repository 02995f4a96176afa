"""Every resource-creation site of the host library is in the failure-injection tour (no GPU needed).

tests/golden/failure_sites.json holds the sites the clean tour of tests/failure_tour.py saw on an MI355X (as the keys of
tests/failure_sites.py); tests/test_gpu_failure_paths.py asserts that the live tour still sees exactly that set and that a
refusal is injected at every one of them.  Here the creator calls found in the sources are held against it: a hipMalloc added
to a host file without a tour step (and a re-recorded golden file) fails this test."""
import json
import os
import re

from failure_sites import CREATORS, HOST_FILES, ROOT, key_of, source_sites

GOLDEN = os.path.join(ROOT, "tests", "golden", "failure_sites.json")

# The sites the tour cannot reach, by name.  Only two reasons count: the site needs a second physical GPU, or it exists only in
# the MRT_STAMPS diagnostic build.
EXCLUDED = {
    "multi_gpu.cpp | HIP_TRY(c, hipMalloc((void**)&c->d_gather_stage, stage_need ? stage_need : 16)); | 1":
        "second GPU: the staging buffer of mrt_gather_rccl is allocated on the root of a communicator of world > 1 only "
        "(one process per GPU)",
}


def test_the_sources_creator_sites_are_the_tours_sites():
    src = set(source_sites().values())
    golden = set(json.load(open(GOLDEN))["sites"])
    assert len(src) >= 60
    assert set(EXCLUDED) <= src, "an excluded site is no longer in the sources"
    assert not golden & set(EXCLUDED), "an excluded site is reached by the tour after all"
    missing = sorted(src - golden - set(EXCLUDED))
    assert not missing, ("creator calls in the host files that the failure-injection tour does not reach (add a step to tests/failure_tour.py and "
                         "record tests/golden/failure_sites.json again on the GPU):\n" + "\n".join(missing))
    gone = sorted(golden - src)
    assert not gone, "sites of tests/golden/failure_sites.json that the sources no longer have (record it again):\n" + "\n".join(gone)


def test_the_search_finds_every_spelling_and_ignores_comments(tmp_path):
    (tmp_path / "x.cpp").write_text(
        "// hipMalloc(&a, 1) in a comment\n"
        "    HIP_TRY(c, hipMalloc(&a, 1));\n"
        "    e = hipHostMalloc (&b, 1, 0);   // hipEventCreate(&e)\n"
        "    if (!s) HIP_TRY(c, hipStreamCreateWithFlags(&s, 1));\n"
        "    if (!s) HIP_TRY(c, hipStreamCreateWithFlags(&s, 1));\n"
        "    hipEventCreate(&e); hipStreamCreate(&s);\n"
        "    my_hipMalloc(&a); hipMallocator(&a); hipFree(a);\n")
    sites = source_sites(str(tmp_path), ("x.cpp",))
    assert sorted(no for _, no in sites) == [2, 3, 4, 5, 6]
    assert sites[("x.cpp", 4)].endswith("| 1") and sites[("x.cpp", 5)].endswith("| 2")
    assert key_of("x.cpp:3 hipHostMalloc", sites) == sites[("x.cpp", 3)] and key_of("x.cpp:1 hipMalloc", sites) is None


def test_the_host_file_list_is_the_librarys():
    """the files searched are the library's host sources and shared headers; the shim is test infrastructure and no source of
    the product (not in the build id's list, not in the product library)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from source_hash import COMPILED, HEADERS, SOURCES
    device_only = ("mrt_device.h", "rt_math.h", "sweep.h", "blend.h")       # headers of the .hip files alone: no host code
    csrc = {os.path.basename(f) for f in COMPILED + HEADERS if f.startswith("myraytracer_amd/csrc/") and not f.endswith(".hip")} - set(device_only)
    assert csrc == set(HOST_FILES)
    assert not [f for f in SOURCES if "failinject" in f or f.startswith("tests/")]
    for f in COMPILED:          # the kernels' files create nothing (they are not routed through the shim)
        if f.endswith(".hip"):
            text = open(os.path.join(ROOT, f)).read()
            assert not re.search(r"\b(" + "|".join(CREATORS) + r")\s*\(", text), f


def test_the_product_library_exports_nothing_of_the_shim(mrt):
    import subprocess
    from myraytracer_amd import _lib
    lib = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd.so")
    names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "mrt_fi_" not in names
    fi = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd_failinject.so")
    assert os.path.exists(fi), "the Makefile's `all` builds the failure-injecting library too"
    names = subprocess.run(["nm", "-D", "--defined-only", fi], capture_output=True, text=True, check=True).stdout
    assert "mrt_fi_arm" in names and all(f" {n}\n" in names for n in _lib.EXPORTS)
