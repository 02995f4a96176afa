"""The library's stream ordering, tested with a slow producer (include/myraytracer_amd.h: frames queued before an update see the
old scene and frames queued after it the new one, the present is queued behind its frame's blend, mrt_present_acquire hands out a
finished image, the framebuffer pointer is a zero-copy hand-off on the caller's stream).

tests/order_walks.py holds the scenarios: each holds one stream of a context with mrt_debug_hold, queues producer and consumer
calls with no sync between them and compares what it reads back with the oracle.  (a) runs every scenario on the product library;
(b) runs them in a child process on the failure-injecting library, once clean and once with each of their hipStreamWaitEvent
calls dropped, and holds the sites at which a dropped wait is detected against tests/golden/order_sites.json (recorded by
`python tests/order_walks.py --scenarios all --log FILE --record tests/golden/order_sites.json` with MRT_LIB_OVERRIDE naming that
library); (c) hands frames to torch on a real torch.cuda.Stream with a sleep kernel pending and nothing but stream.synchronize()."""
import json
import os

import numpy as np
import pytest

import order_walks as OW
from common import mismatch_report, oracle_render
from failure_sites import ROOT, run_child

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "order_sites.json")
SLEEP_CYCLES = 400_000_000          # ~0.2 s (tests/test_gpu_multi.py's)


@pytest.fixture(scope="module")
def env(mrt, oracle):
    return OW.Env(mrt, oracle)


def test_the_hold_creates_nothing_and_both_its_bounds_end_it(mrt, env):
    """mrt_debug_hold refuses a stream the context does not have yet, ticks above its cap and no polls; a hold of the cap's
    ticks and one poll ends at once (its stamps less than a millisecond apart), one of many polls after its ticks"""
    from myraytracer_amd import _lib
    sc = OW.Scenario(env, "hold")
    with sc.state() as st:
        for which, index in (("present", 0), ("noise", 0), ("slot", 15)):
            with pytest.raises(mrt.MrtError) as e:
                st.debug_hold(which, index, 1000, 1000)
            assert e.value.status == 7, which
        for args in (("context", 0, _lib.HOLD_MAX_TICKS + 1, 1000), ("context", 0, 0, 1000), ("context", 0, 1000, 0), ("context", 1, 1000, 1000),
                     ("slot", 16, 1000, 1000)):
            with pytest.raises(mrt.MrtError) as e:
                st.debug_hold(*args)
            assert e.value.status == 1, args
        assert st.debug_hold_stamps() == (0, 0, 0)
        assert st.debug_check_context() is None
        st.debug_hold("context", 0, _lib.HOLD_MAX_TICKS, 1)
        st.sync()
        start, end, polls = st.debug_hold_stamps()
        assert polls == 1 and 0 <= end - start < 100_000, (start, end)
        st.redraw()
        st.debug_hold("slot", 0, 20_000, 1 << 20)
        st.sync()
        start, end, polls = st.debug_hold_stamps()
        assert polls == 1 << 20 and 20_000 <= end - start < 120_000, (start, end)


@pytest.mark.parametrize("name", list(OW.SCENARIOS))
def test_the_scenario_equals_its_reference_with_a_stream_held(env, name):
    """(a) the product library, nothing dropped: the observable is the reference's bit for bit, counters included"""
    rec = OW.run_case(env, OW.SCENARIOS[name](env, name))
    print(rec)
    assert not rec["findings"], rec["findings"]
    assert not rec["differs"], f"{name}: {rec['differs']} differ from the reference"


@pytest.mark.parametrize("group", list(OW.GROUPS))
def test_a_dropped_stream_wait_is_detected(group, tmp_path):
    """(b) every scenario of the group clean (it equals its reference) and with each of its W stream waits dropped in turn; the
    sites at which the recorded run detected the drop in a scenario of this group are detected again"""
    recs = run_child(os.path.join(ROOT, "tests", "order_walks.py"), ["--scenarios", group], tmp_path / "order.jsonl", 120)
    findings = [f"{r['scenario']} N={r['n']}: {f}" for r in recs for f in r.get("findings", [])]
    assert not findings, f"{len(findings)} findings, the first of them:\n" + "\n".join(findings[:20])
    for name in OW.GROUPS[group]:
        mine = [r for r in recs if r.get("scenario") == name]
        assert mine and mine[0].get("mode") == "clean" and not mine[0]["differs"], name
        assert [r["n"] for r in mine[1:]] == list(range(1, mine[0]["waits"] + 1)), name
        assert all(r["site"] for r in mine[1:]), name
    detected = OW.detected_sites(recs)
    for r in recs:
        if r.get("n"):
            print(f"{r['scenario']} N={r['n']} {r['site']}: {'detected ' + str(r['differs']) if r['detected'] else 'not detected'}")
    golden = json.load(open(GOLDEN))["sites"]
    for key, scenarios in golden.items():           # every scenario built to miss a wait still does
        for name in set(scenarios) & set(OW.GROUPS[group]):
            assert name in detected.get(key, ()), f"{name} no longer detects a dropped wait at {key}"
    for key, scenarios in detected.items():
        assert set(scenarios) <= set(golden.get(key, ())), f"{key}: {scenarios} detect it and the golden file does not say so (record it again)"


def _state(mrt, env, stream):
    sc = OW.Scenario(env, "torch")
    sc.slots = 0                    # (the library's own schedule)
    return sc, sc.state(stream=stream.cuda_stream)


def test_a_clone_on_the_callers_stream_behind_a_sleep_is_the_frame(mrt, env):
    """(c) a sleep kernel pending on the caller's stream, then set_world, redraw and a clone of the zero-copy tensor: after
    stream.synchronize() alone the clone is the oracle's frame"""
    import torch
    from myraytracer_amd import dist as mdist
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sc, st = _state(mrt, env, stream)
        with st:
            torch.cuda._sleep(SLEEP_CYCLES)
            st.set_world(sc.old)
            st.redraw()
            snap = mdist.framebuffer_tensor(st).clone()
            stream.synchronize()
            got = snap.cpu().numpy()[:OW.H]         # (the tensor's rows are whole bands: the image's come first)
    ref, _ = env.frames([(sc.old, sc.cam)])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), mismatch_report(got, ref)


def test_a_snapshot_behind_a_sleep_survives_two_more_frames(mrt, env):
    """(c) a clone of frame 1 queued behind a sleep, then two more redraws -- the second of which blends into the buffer the
    clone reads: the snapshot is still frame 1 and the framebuffer the oracle's three frames"""
    import torch
    from myraytracer_amd import dist as mdist
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sc, st = _state(mrt, env, stream)
        with st:
            st.redraw()
            view = mdist.framebuffer_tensor(st)
            torch.cuda._sleep(SLEEP_CYCLES)
            snap = view.clone()
            st.redraw()
            st.redraw()
            assert mdist.framebuffer_tensor(st).data_ptr() == view.data_ptr(), "the ping-pong is back on the snapshot's buffer"
            stream.synchronize()
            got1, got3 = snap.cpu().numpy()[:OW.H], st.read_framebuffer()
    ref1, _ = env.frames([(sc.old, sc.cam)])
    ref3, _ = env.frames([(sc.old, sc.cam)] * 3)
    assert np.array_equal(got1.view(np.uint32), ref1.view(np.uint32)), "the reader saw a later frame: " + mismatch_report(got1, ref1)
    assert np.array_equal(got3.view(np.uint32), ref3.view(np.uint32)), mismatch_report(got3, ref3)


def test_switching_streams_in_the_middle_of_an_accumulation(mrt, env):
    """(c) mrt_set_stream from one torch stream to another with a sleep and a frame pending on the old one: the accumulation
    over both streams is the oracle's five frames, with the counters"""
    import torch
    from myraytracer_amd import _lib
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    sc, st = _state(mrt, env, first)
    with st:
        with torch.cuda.stream(first):
            st.redraw()
            st.redraw()
            torch.cuda._sleep(SLEEP_CYCLES)
            st.redraw()
        st._check(_lib.load().mrt_set_stream(st._ctx, second.cuda_stream), "mrt_set_stream")
        with torch.cuda.stream(second):
            st.redraw()
            st.redraw()
            second.synchronize()
        got, counters = st.read_framebuffer(), st.read_counters()
    ref, ref_counters = env.frames([(sc.old, sc.cam)] * 5)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), mismatch_report(got, ref)
    assert {k: counters[k] for k in OW.COUNTER_KEYS} == ref_counters


def test_zero_copy_framebuffer_tensor_on_a_real_stream(mrt, oracle):
    """(c) tests/test_gpu_golden_and_api.py::test_zero_copy_framebuffer_tensor on a torch.cuda.Stream made current, whose handle
    is not 0, and without the device-wide synchronise: torch's op on the tensor follows the redraw by stream order alone"""
    import torch
    from myraytracer_amd import dist as mdist
    sc = mrt.scene_default()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        with mrt.State(mrt.Args(40, 24, 2, 8), seed=1, stream=stream.cuda_stream) as st:
            st.set_world(sc)
            st.redraw()
            t = mdist.framebuffer_tensor(st)
            assert t.is_cuda and tuple(t.shape) == (24, 40, 4)
            img = mdist.gather_framebuffer(t, 24)
            stream.synchronize()
            got = img.cpu().numpy()
            assert np.array_equal(got, st.read_framebuffer())
    ref = oracle_render(oracle, sc, None, 40, 24, 2, 8, 1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), mismatch_report(got, ref)
