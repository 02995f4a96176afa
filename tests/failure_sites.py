"""The resource-creation sites of the host library, named so that the names survive edits elsewhere in a file.

A site is a source line of a host file that calls one of the six creators.  The failure-injecting build (tests/failinject/)
reports a site as "file.cpp:LINE hipName"; a line number moves with every edit above it, so tests/golden/failure_sites.json and
the comparisons use a key instead: "file.cpp | <the line's code, stripped> | k", k counting identical lines within the file.
Used by tests/failure_tour.py (on the GPU machine) and tests/test_failure_sites.py (without a GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myraytracer_amd", "csrc")
# the host files (scripts/source_hash.py's compiled .cpp files and the headers they share)
HOST_FILES = ("api.cpp", "frames.cpp", "world.cpp", "noise.cpp", "present.cpp", "denoise.cpp", "multi_gpu.cpp", "hierarchy.cpp",
              "scenes.cpp", "image_io.cpp", "mrt_ctx.h", "mrt_internal.h", "hierarchy.h", "bounds.h", "width_policy.h")
CREATORS = ("hipMalloc", "hipHostMalloc", "hipStreamCreate", "hipStreamCreateWithFlags", "hipEventCreate", "hipEventCreateWithFlags")
_CALL = re.compile(r"\b(" + "|".join(sorted(CREATORS, key=len, reverse=True)) + r")\s*\(")


def _code(line):
    """The line without its // comment (no creator call here shares a line with a string that holds "//")."""
    return line.split("//", 1)[0].strip()


def source_sites(csrc=CSRC, files=HOST_FILES):
    """{(file, line number): key} for every creator call in the host files; a line with two calls is one site."""
    sites = {}
    for name in files:
        seen = {}
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                code = _code(line)
                if code.startswith("#define") or not _CALL.search(code):
                    continue
                k = seen[code] = seen.get(code, 0) + 1
                sites[(name, no)] = f"{name} | {code} | {k}"
    return sites


def key_of(shim_site, sites=None):
    """The key of a site as the shim reports it ("file.cpp:LINE hipName"); None if the sources have no creator call there."""
    sites = source_sites() if sites is None else sites
    where = shim_site.split(" ", 1)[0]
    name, _, no = where.rpartition(":")
    return sites.get((name, int(no)))
