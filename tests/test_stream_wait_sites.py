"""Every hipStreamWaitEvent of the host library is one whose loss a stream-ordering scenario notices (no GPU needed).

tests/golden/order_sites.json holds the sites (as the keys of tests/failure_sites.py) at which tests/order_walks.py, run on an
MI355X against the failure-injecting library, dropped the wait and saw some scenario's observable leave its reference, with the
scenarios that saw it; tests/test_gpu_stream_order.py asserts that the live walks still detect them.  Here the stream waits found
in the sources are held against that file: a wait added to a host file without a scenario that misses it fails this test."""
import json
import os

from failure_sites import ROOT, WAITS, key_of, source_sites

GOLDEN = os.path.join(ROOT, "tests", "golden", "order_sites.json")

# The sites no scenario can detect, by name.  Only three reasons count: the site needs a second physical GPU; the wait is implied,
# in every program order the API allows, by other waits (named, with the argument); dropping it could change an address a kernel
# reads.  At most three.
EXCLUDED = {
    "world.cpp | const hipError_t e = hipStreamWaitEvent(c->stream, S.render_done, 0); | 1":
        "implied by frames.cpp, launch_frame: `HIP_TRY(c, hipStreamWaitEvent(c->stream, S.render_done, 0));`.  render_done is "
        "recorded in launch_frame alone, and the very next runtime call there makes the context's stream wait for it; "
        "order_behind_frames runs later on the host, for the same c->stream (mrt_set_stream, the one call that changes it, first "
        "waits on the host for every frame and clears render_pending), so each slot it finds pending is one whose render_done the "
        "context's stream already waits for, ahead of whatever the scatter queues.  The walks show it: with this wait dropped "
        "every scatter scenario still equals its reference, with launch_frame's dropped none does.",
    "noise.cpp | HIP_TRY(c, hipStreamWaitEvent(c->noise_stream, c->noise_ring[seq % kNoiseRing].copied, 0)); | 1":
        "implied by a wait on the host for the same event: mrt_render_adaptive reaches it only with `seq` a report whose "
        "`copied` it has just seen complete -- report_seq 0 takes the newest for which hipEventQuery returned hipSuccess, any "
        "other report_seq goes through mrt::wait_event(c, ...copied) -- and an entry's event is recorded again only by a later "
        "mrt_noise_query on the same host thread.  The sibling wait of mrt_read_noise_tiles, which has no such host wait, is "
        "covered (noise/context, noise/noise).",
}


def test_the_sources_stream_waits_are_detected_or_excluded_with_a_reason():
    src = set(source_sites(calls=WAITS).values())
    golden = json.load(open(GOLDEN))["sites"]
    assert len(src) >= 10
    assert len(EXCLUDED) <= 3 and all(len(why) > 80 for why in EXCLUDED.values())
    assert set(EXCLUDED) <= src, "an excluded site is no longer in the sources"
    assert not set(golden) & set(EXCLUDED), "a dropped wait at an excluded site is detected after all"
    assert all(golden.values()), "a recorded site names no scenario"
    missing = sorted(src - set(golden) - set(EXCLUDED))
    assert not missing, ("stream waits in the host files that no scenario of tests/order_walks.py misses when they are dropped (add a scenario and "
                         "record tests/golden/order_sites.json again on the GPU):\n" + "\n".join(missing))
    gone = sorted(set(golden) - src)
    assert not gone, "sites of tests/golden/order_sites.json that the sources no longer have (record it again):\n" + "\n".join(gone)


def test_the_recorded_scenarios_exist():
    import order_walks
    golden = json.load(open(GOLDEN))["sites"]
    for key, scenarios in golden.items():
        assert set(scenarios) <= set(order_walks.SCENARIOS), key
    assert sorted(n for g in order_walks.GROUPS.values() for n in g) == sorted(order_walks.SCENARIOS), "every scenario is in one group"


def test_the_search_takes_a_call_name_and_ignores_comments(tmp_path):
    (tmp_path / "x.cpp").write_text(
        "// hipStreamWaitEvent(s, e, 0) in a comment\n"
        "    HIP_TRY(c, hipStreamWaitEvent(s, e, 0));\n"
        "    e = hipStreamWaitEvent (s, e, 0);   // hipStreamWaitEvent(s, e, 0)\n"
        "    HIP_TRY(c, hipStreamWaitEvent(s, e, 0));\n"
        "    HIP_TRY(c, hipMalloc(&a, 1)); my_hipStreamWaitEvent(s); hipStreamWaitEvents(s);\n"
        "#define hipStreamWaitEvent(...) routed(__VA_ARGS__)\n")
    sites = source_sites(str(tmp_path), ("x.cpp",), calls=WAITS)
    assert sorted(no for _, no in sites) == [2, 3, 4]
    assert sites[("x.cpp", 2)] == "x.cpp | HIP_TRY(c, hipStreamWaitEvent(s, e, 0)); | 1" and sites[("x.cpp", 4)].endswith("| 2")
    assert key_of("x.cpp:3 hipStreamWaitEvent", sites) == sites[("x.cpp", 3)] and key_of("x.cpp:1 hipStreamWaitEvent", sites) is None
    assert sorted(no for _, no in source_sites(str(tmp_path), ("x.cpp",))) == [5], "the default is still the creators"
